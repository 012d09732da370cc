"""One process of tests/test_gpu_blur_reference.py: the kernels that launch_blur_clip keeps behind environment switches (the library reads
some of them once per process) against the float64 reference of tests/blur_ref.py.  The parent sets the switch in this process's
environment.  usage: blur_ab_worker.py runtime | unrolled
  runtime   the stripr and ring rows of the table, and their frames with NaN and Inf samples   (LSPIV_BLUR_BLOCK=1, LSPIV_BLUR_RING=1)
  unrolled  the strip4 row of the table                                                       (LSPIV_BLUR_ONE_COLUMN=1)
Prints one JSON line: the number of results compared, those whose masks or gate failed, the largest error / gate."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyorc_amd import _lib, filters  # noqa: E402
from tests import blur_ref as br  # noqa: E402

_lib.require_device()
rows = ("stripr", "ring") if sys.argv[1] == "runtime" else ("strip4",)
n, failed, worst = 0, [], 0.0


def check(kind, key, dt, w, fam):
    global n, worst
    fr = br.STACKS[kind](key, dt)
    w1, w2 = br.split(w)
    got = filters.smooth(fr, w1) if w2 is None else filters.edge_detect(fr, w1, w2)
    masks, ratio = br.compare(got, br.reference(kind, key, dt, w), fr, w)
    n += 1
    worst = max(worst, ratio)
    if br.family(dt, w1, w2, fr.shape[2]) != fam or not masks or not ratio <= 1.0:        # the family the switch's kernel stands in for
        failed.append([kind, str(key), dt, str(w), masks, ratio])


for row in rows:
    windows, shapes = br.TABLE[row]
    for shape, dtypes in shapes:
        for dt in dtypes:
            for w, fam in windows.items():
                check("table", shape, dt, w, fam)
    if row != "strip4":
        for dt in br.F:
            for w, fam in windows.items():
                check("nonfinite", row, dt, w, fam)
print(json.dumps({"n": n, "failed": failed, "worst": worst if np.isfinite(worst) else 1e30}))
