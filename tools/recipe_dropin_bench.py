"""The recipe's ``frames:`` section inside the pyorc drop-in, timed: normalize(15) -> edge_detect(1, 2) -> minmax(-5, 5) -> project(hip)
-> get_piv(hip) on a lazy 1080p uint8 camera stack in 20-frame blocks (tests/recipe_doubles.py: pyorc's Frames with the filters as
per-block layers over tests/lazy_doubles.py), projected to 810 x 1440, 201 frames = 200 pairs, 32 x 32 windows at 16.  Prints one JSON
line with pairs/s of

  (a) the chain drop-in: uint8 camera blocks loaded, the filters run on the device before the projection;
  (b) today's path on the same recipe: the double's CPU filters compute the blocks, the float32 camera frames feed the hand-off;
  (c) today's uint8 hand-off with no filters at all;

and, for each, the split ``LAST_STATS`` reports (load, upload + filters + projection, launch, waited for loads)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyorc_amd import _lib, executor, frames as F, plugin  # noqa: E402
from pyorc_amd.synth import particle_stack, projection_maps  # noqa: E402
from tests import lazy_doubles, recipe_doubles as rd  # noqa: E402

T, SRC, DST = 201, (1080, 1920), (810, 1440)
WS, OV = 32, (16, 16)


def main():
    _lib.require_device()
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    sys.modules["xarray"] = lazy_doubles
    saved = {}

    def setitem(d, k, v):
        saved.setdefault(k, d.get(k))
        d[k] = v

    rd.install(setitem)
    cam = particle_stack(T, SRC[0], SRC[1], seed=5)
    maps = projection_maps(SRC, DST, tilt=0.1, seed=1)
    t = np.arange(T) / 30.0
    Fr = rd.Frames

    def graph(kind):
        root = rd.camera(cam, block=20)
        stack = root if kind == "c" else Fr(Fr(Fr(root).normalize(15)).edge_detect(1, 2)).minmax(-5, 5)
        if kind == "b":
            plugin._FILTERS.clear()     # nothing recorded: what an unpatched pyorc hands over today
        return lazy_doubles.frames_project(stack, maps, DST, plugin.project_hip)

    out = {"frames": T, "camera": list(SRC), "ortho": list(DST), "window": WS, "overlap": list(OV), "block": 20}
    results = {}
    try:
        for kind, label, n in (("a", "chain_dropin", repeats), ("b", "todays_path_cpu_filters", 1), ("c", "uint8_handoff_no_filters", repeats)):
            F.get_piv(graph(kind), WS, overlap=OV, time=t, resolution=0.01)          # warm: workspaces, pinned ring, plans
            walls = []
            for _ in range(n):
                g = graph(kind)           # graph building (normalize's sampled mean on the host) is not timed: the recipe builds it once
                t0 = time.perf_counter()
                results[kind] = F.get_piv(g, WS, overlap=OV, time=t, resolution=0.01)
                walls.append(time.perf_counter() - t0)
                st = dict(executor.LAST_STATS)
            wall = float(np.median(walls))
            out[f"{kind}_{label}_pairs_per_s"] = round((T - 1) / wall, 1)
            out[f"{kind}_detail"] = {"wall_s": [round(w, 4) for w in walls], "chain": st["plan"].get("chain"), "loads": st.get("chunks"),
                                     "load_s": st.get("load_s"), "upload_filter_project_s": st.get("upload_s"),
                                     "launch_s": st.get("launch_s"), "waited_for_loads_s": st.get("waited_s"),
                                     "normalize_mean_s": st.get("mean_s")}
    finally:
        plugin.uninstall()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    out["a_over_c"] = round(out["a_chain_dropin_pairs_per_s"] / out["c_uint8_handoff_no_filters_pairs_per_s"], 3)
    out["a_over_b"] = round(out["a_chain_dropin_pairs_per_s"] / out["b_todays_path_cpu_filters_pairs_per_s"], 2)
    # (a) and (b) compute the same recipe; (b) through the oracle's restated GaussianBlur on the host, (a) through the kernels: equal to
    # the last float32 bits is not expected there, so report the largest difference of the velocities instead
    out["a_vs_b_max_abs_v_diff"] = float(max(np.nanmax(np.abs(results["a"][k] - results["b"][k])) for k in ("v_x", "v_y")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
