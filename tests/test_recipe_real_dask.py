"""The recipe's filter chain (pyorc_amd.plugin's recorded Frames filters) on a REAL dask graph: tests/recipe_dask_worker.py, run by the
interpreter of the build image that has dask (as tests/test_real_dask.py does); skipped where that interpreter or its dask is missing."""
import os
import subprocess

import pytest

from tests.test_real_dask import CONDA_PY, ROOT, SYSTEM_LIBSTDCXX, _has_dask


@pytest.mark.skipif(not _has_dask(), reason="no interpreter with dask in this image")
def test_the_recipe_chain_resolves_on_a_real_dask_graph():
    """What it asserts (tests/recipe_dask_worker.py): the names recorded for pyorc's normalize (astype / sub / min / max / astype), its
    apply_ufunc edge_detect and its np.maximum(np.minimum()) minmax are the layer names of the real HighLevelGraph, the chain under
    project_hip resolves to the uint8 root there, and get_piv runs it without dask computing a filter block -- with the bits of today's
    path on the same graph."""
    env = dict(os.environ, LSPIV_NO_AUTO_INSTALL="1")
    if os.path.exists(SYSTEM_LIBSTDCXX):
        env["LD_PRELOAD"] = SYSTEM_LIBSTDCXX + (":" + env["LD_PRELOAD"] if env.get("LD_PRELOAD") else "")
    r = subprocess.run([CONDA_PY, "-W", "ignore", os.path.join(ROOT, "tests", "recipe_dask_worker.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "OK recipe dask" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
