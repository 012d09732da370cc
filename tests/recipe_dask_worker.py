"""The recipe's filter chain against a REAL dask (run by tests/test_recipe_real_dask.py under the interpreter of the build image that has
dask; xarray is nowhere, so the DataArray around a dask array is the wrapper of tests/real_dask_worker.py).

What is real: the graphs pyorc's filters build -- ``normalize``'s ``astype`` / ``sub`` / ``min`` / ``max`` / ``astype`` (pyorc/api/frames.py:
296-306), ``edge_detect`` / ``smooth`` as ``xr.apply_ufunc(..., dask="parallelized")`` (= ``dask.array.apply_gufunc``), ``minmax``'s
``np.maximum(np.minimum(...))`` (:362) --, their names, ``HighLevelGraph.dependencies``, the threaded scheduler.  What is a double: the GPU
(the oracle computes the chain, the projection and the PIV on host stacks)."""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["LSPIV_NO_AUTO_INSTALL"] = "1"

import dask  # noqa: E402
import dask.array as da  # noqa: E402

from oracle import filters_oracle as fo  # noqa: E402
from pyorc_amd import _lib, executor, frames as F, plugin, velocimetry as V  # noqa: E402
from pyorc_amd.synth import particle_stack, projection_maps  # noqa: E402
from tests import doubles, recipe_doubles as rd  # noqa: E402
from tests.real_dask_worker import Lazy, Setattr  # noqa: E402
from tests.test_round6_host import OraclePlan  # noqa: E402

BLUR_CALLS = []
_lock = threading.Lock()


def _edges(block, wdw_1, wdw_2):
    with _lock:
        BLUR_CALLS.append(len(block))
    return fo.edge_detect(block, wdw_1, wdw_2) if len(block) else np.zeros(block.shape, np.float32)


class DaskFrames:
    """pyorc's filter methods on a dask-backed stack, the expressions of pyorc/api/frames.py."""

    def __init__(self, obj):
        self._obj = obj

    def normalize(self, samples=15):
        x = self._obj.data
        time_interval = round(len(x) / samples)
        mean = x[::time_interval].mean(axis=0).compute(scheduler="threads").astype("float32")
        frames_reduce = x.astype("float32") - mean
        frames_min = frames_reduce.min(axis=-1).min(axis=-1)[:, None, None]
        frames_max = frames_reduce.max(axis=-1).max(axis=-1)[:, None, None]
        return Lazy(((frames_reduce - frames_min) / (frames_max - frames_min) * 255).astype("uint8"))

    def edge_detect(self, wdw_1=1, wdw_2=2):
        return Lazy(da.apply_gufunc(_edges, "(y,x)->(y,x)", self._obj.data, output_dtypes=np.float32, wdw_1=wdw_1, wdw_2=wdw_2))

    def minmax(self, min=-np.inf, max=np.inf):
        return Lazy(np.maximum(np.minimum(self._obj.data, max), min))

    def smooth(self, wdw=1):
        return Lazy(da.apply_gufunc(lambda b: fo.smooth(b, wdw) if len(b) else b.astype(np.float32), "(y,x)->(y,x)", self._obj.data,
                                    output_dtypes=np.float32))

    def get_piv(self, *args, **kwargs):
        raise NotImplementedError


def main():
    mp = Setattr()
    mp.setattr(V.piv, "piv_pairs", doubles.oracle_piv_pairs)
    mp.setattr(V.window, "available_memory", lambda: 1e12)
    mp.setattr(V.window, "chunk_alignment", lambda ws, dim=None, ov=None: 10)
    mp.setattr(_lib, "require_device", lambda: None)
    from pyorc_amd import project as P

    mp.setattr(P, "Projection", OraclePlan)
    doubles.use_host_stacks(mp)
    seen = []
    rd.host_chain(mp, seen)
    rd.install(lambda d, k, v: d.__setitem__(k, v), DaskFrames)
    src, dst = (96, 128), (72, 100)
    maps = projection_maps(src, dst, tilt=0.2, seed=4)
    cam = particle_stack(47, src[0], src[1], seed=12)
    t = np.arange(47) / 30.0
    root = Lazy(da.from_array(cam, chunks=(10,) + src))
    n = DaskFrames(root).normalize(15)
    e = DaskFrames(n).edge_detect(1, 2)
    m = DaskFrames(e).minmax(-5, 5)
    # the names recorded are those of the results' dask arrays: pyorc's expressions end in astype / the gufunc / maximum
    rec = {k: v[0] for k, v in plugin._FILTERS.items()}
    assert rec == {n.data.name: "normalize", e.data.name: "edge_detect", m.data.name: "minmax"}, rec
    assert n.data.name.startswith("astype-") and m.data.name.startswith("maximum-"), (n.data.name, m.data.name)
    # ... and what the walk meets on the real HighLevelGraph: each recorded name is a layer, its source's name the layer below
    for res, below in ((m, e), (e, n)):
        assert res.data.name in res.data.dask.layers and below.data.name in res.data.dask.layers
    plan_args = tuple(maps)
    ortho = da.apply_gufunc(plugin._project_block, "(y,x)->(ny,nx)", m.data, output_dtypes=np.float32, output_sizes={"ny": dst[0], "nx": dst[1]},
                            plan_args=plan_args, dst_shape=dst, device=None)
    plugin._register_projection(Lazy(ortho), m, plan_args, dst, None)
    filled = Lazy(da.where(~da.isnan(ortho), ortho, 0.0))
    hit = plugin.hip_projection_source(filled)
    assert hit is not None and hit["root"] is root and [op for op, _ in hit["ops"]] == ["normalize", "edge_detect", "minmax"], hit
    assert hit["ops"][1][1] == {"wdw_1": 1, "wdw_2": 2} and hit["ops"][2][1] == {"min": -5.0, "max": 5.0}
    # the drop-in run on the real graph: no block of the filters computed by dask, uint8 camera blocks handed to the chain
    BLUR_CALLS.clear()
    got = F.get_piv(filled, 32, time=t, resolution=0.01)
    st = dict(executor.LAST_STATS)
    assert st["plan"]["chain"] == ["normalize", "edge_detect", "minmax"] and st["plan"]["source"] == "camera", st["plan"]
    assert BLUR_CALLS == [] and seen and all(dt == np.uint8 for dt in seen), (BLUR_CALLS, seen)
    # today's path on the same graph (nothing recorded): dask computes the filters; the same bits
    plugin._FILTERS.clear()
    ref = F.get_piv(filled, 32, time=t, resolution=0.01)
    assert "chain" not in executor.LAST_STATS["plan"] and sum(BLUR_CALLS) == 47, BLUR_CALLS
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    plugin.uninstall()
    mp.undo()
    print("OK recipe dask", dask.__version__)


if __name__ == "__main__":
    main()
