"""A pyorc double for the recipe's ``frames:`` section (normalize -> edge_detect -> minmax, or smooth) ahead of ``project`` -> ``get_piv``.

* :class:`Stack` is ``tests/lazy_doubles.LazyDataArray`` that also takes step slices along time (``frames[::n]``, what ``normalize``
  samples, pyorc/api/frames.py:296-299) and keeps its class through the graph-building operations;
* :class:`Frames` has the four filter methods of pyorc's accessor (frames.py:279-467) with the reference's names and defaults, plus
  ``time_diff`` (frames.py:409-436), built on ``oracle/filters_oracle.py``.  Each filter is a per-block layer named after it; the blocks
  it computes are counted in the stack's ``calls`` (``filter_blocks``).  ``made`` holds every result, in order;
* :func:`fake_pyorc` is the package ``pyorc_amd.plugin.install`` patches, with this ``Frames`` in ``pyorc.api.frames``.
"""
import sys
import types

import numpy as np

from oracle import filters_oracle as fo
from tests import fake_xarray, lazy_doubles

FILTER_LAYERS = ("normalize", "edge_detect", "minmax", "smooth")


class Stack(lazy_doubles.LazyDataArray):
    def _like(self, **kw):
        out = super()._like(**kw)
        out.__class__ = Stack
        return out

    def __getitem__(self, key):
        if isinstance(key, slice) and key.step not in (None, 1):
            a, b, step = key.indices(len(self))
            return _Strided(super().__getitem__(slice(a, b)), step)
        return super().__getitem__(key)


class _Strided:
    """``frames[a:b:step]``: like dask, computes the blocks that hold a selected frame, one at a time, and keeps only those frames."""

    def __init__(self, base, step):
        self._base, self._step = base, step

    def __len__(self):
        return -(-len(self._base) // self._step)

    def load(self):
        edges = np.concatenate([[0], np.cumsum(self._base.chunks[0])]).astype(int)
        parts = []
        for e0, e1 in zip(edges, edges[1:]):
            sel = [i - e0 for i in range(-(-e0 // self._step) * self._step, e1, self._step)]
            if sel:
                parts.append(self._base[e0:e1].load().values[sel])
        return fake_xarray.DataArray(np.concatenate(parts), self._base.dims)


def camera(frames, block=20, layer=None):
    """A lazy ``(time, y, x)`` stack in blocks of ``block`` frames (a video opened by pyorc); ``layer``: a counted identity layer of that
    name on top (the decode of the blocks)."""
    T = len(frames)
    blocks = list(range(0, T, block)) + [T]
    root = Stack(frames, blocks, frames.shape[1:], frames.dtype, coords={"time": np.arange(T) / 30.0})
    return root if layer is None else root.map_time(lambda blk: blk, layer)


def filter_blocks(stack, prefixes=FILTER_LAYERS):
    """(layer prefix, block) -> computations of the filter layers of ``stack``'s graph."""
    return {(k[0].rsplit("-", 1)[0], k[1]): v for k, v in stack.calls.items() if k[0].rsplit("-", 1)[0] in prefixes}


class Frames:
    """``frames.frames``: the accessor around a lazy stack (``_obj``)."""

    made = []

    def __init__(self, obj):
        self._obj = obj

    def _out(self, out):
        Frames.made.append(out)
        return out

    def normalize(self, samples=15):
        time_interval = round(len(self._obj) / samples)
        assert time_interval != 0, f"Amount of frames is too small to provide {samples} samples"
        mean = self._obj[::time_interval].load().values.mean(axis=0).astype("float32")     # computed when the graph is built, as there
        return self._out(self._obj.map_time(lambda blk: fo.normalize_with_mean(blk, mean), "normalize", dtype=np.uint8))

    def edge_detect(self, wdw_1=1, wdw_2=2):
        return self._out(self._obj.map_time(lambda blk: fo.edge_detect(blk, wdw_1, wdw_2), "edge_detect", dtype=np.float32))

    def minmax(self, min=-np.inf, max=np.inf):
        return self._out(self._obj.map_time(lambda blk: fo.minmax(blk, min, max), "minmax", dtype=np.float32))

    def smooth(self, wdw=1):
        return self._out(self._obj.map_time(lambda blk: fo.smooth(blk, wdw), "smooth", dtype=np.float32))

    def time_diff(self, thres=0, abs=False):
        """One frame fewer: not a per-block layer.  Computed when it is called (what matters here is that it is not recorded)."""
        d = fo.time_diff(self._obj.load().values, thres, abs)
        out = Stack(d, list(range(0, len(d), 20)) + [len(d)], d.shape[1:], d.dtype, coords={"time": np.arange(len(d)) / 30.0},
                    name=lazy_doubles._name("time_diff"), calls=self._obj.calls)
        return self._out(out)

    def get_piv(self, window_size=None, overlap=None, engine="numba", ensemble_corr=False, **kwargs):
        raise NotImplementedError("the tests call pyorc_amd.frames.get_piv directly")


def fake_pyorc(frames_cls=None):
    """``{module name: module}`` of a package ``pyorc`` with ``frames_cls`` (default :class:`Frames`) in ``pyorc.api.frames`` (what
    ``install`` needs)."""
    pyorc = types.ModuleType("pyorc"); pyorc.__path__ = []
    api = types.ModuleType("pyorc.api"); api.__path__ = []
    velo = types.ModuleType("pyorc.velocimetry"); velo.__path__ = []
    ffpiv = types.ModuleType("pyorc.velocimetry.ffpiv")
    frames = types.ModuleType("pyorc.api.frames")
    project = types.ModuleType("pyorc.project")

    def get_ffpiv(frames_, y, x, dt, window_size, overlap, search_area_size, res_y, res_x, chunksize=None, memory_factor=4,
                  engine="numba", ensemble_corr=False, corr_min=0.2, s2n_min=3, count_min=0.2, signal_threshold=None):
        raise NotImplementedError

    ffpiv.get_ffpiv = velo.get_ffpiv = get_ffpiv
    velo.ffpiv = ffpiv
    frames.Frames = Frames if frames_cls is None else frames_cls
    pyorc.api, pyorc.velocimetry, pyorc.project, api.frames = api, velo, project, frames
    return {"pyorc": pyorc, "pyorc.api": api, "pyorc.api.frames": frames, "pyorc.velocimetry": velo, "pyorc.velocimetry.ffpiv": ffpiv,
            "pyorc.project": project}


def install(setitem, frames_cls=None):
    """Put :func:`fake_pyorc` into ``sys.modules`` through ``setitem(sys.modules, name, module)`` (pytest's ``monkeypatch.setitem``) and
    run ``pyorc_amd.plugin.install`` on it.  Returns the package."""
    from pyorc_amd import plugin

    plugin.uninstall()
    mods = fake_pyorc(frames_cls)
    for k, v in mods.items():
        setitem(sys.modules, k, v)
    assert plugin.install(mods["pyorc"])
    return mods["pyorc"]


def host_chain(monkeypatch, seen=None):
    """``pyorc_amd.filters.Chain`` computed by the oracle on the ``tests/doubles.HostStack`` pieces (CPU tests of the drop-in: no HBM).
    ``seen``: a list that receives the dtype of every piece the chain is handed."""
    from pyorc_amd import filters

    from tests.doubles import HostStack

    def mean_plane(self, sampled):
        return HostStack(np.asarray(sampled).mean(axis=0).astype("float32")[None])

    def apply(self, frames, mean=None):
        a = np.asarray(frames)
        if seen is not None:
            seen.append(a.dtype)
        for op, p in self.ops:
            if op == "normalize":
                a = fo.normalize_with_mean(a, np.asarray(mean)[0])
            elif op == "edge_detect":
                a = fo.edge_detect(a, p["wdw_1"], p["wdw_2"]).astype(np.float32)
            elif op == "smooth":
                a = fo.smooth(a, p["wdw"]).astype(np.float32)
            else:
                a = fo.minmax(a, p["min"], p["max"])
        return HostStack(np.ascontiguousarray(a))

    monkeypatch.setattr(filters.Chain, "mean_plane", mean_plane)
    monkeypatch.setattr(filters.Chain, "apply", apply)
