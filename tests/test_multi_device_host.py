"""get_ffpiv(devices=...) without a GPU: resolving the keyword, cutting the pairs over device workers, the lazy plan per device, the
keyword through the pyorc drop-in, and the ABI of the device-side ensemble reduction."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---- the keyword ------------------------------------------------------------------------------------------------------------------
def test_resolve_devices_accepts_none_all_and_lists_with_repeats():
    from pyorc_amd.executor import resolve_devices

    assert resolve_devices(None, 8) is None
    assert resolve_devices("all", 8) == list(range(8))
    assert resolve_devices("all", 1) == [0]
    assert resolve_devices([0, 0], 1) == [0, 0]
    assert resolve_devices((2, 0, 2), 3) == [2, 0, 2]
    assert resolve_devices(np.array([1, 0]), 2) == [1, 0]


@pytest.mark.parametrize("bad", [[], [8], [-1], [0, 1.0], ["0"], [True], "some", 3, [None]])
def test_resolve_devices_rejects_what_names_no_device(bad):
    from pyorc_amd.executor import resolve_devices

    with pytest.raises(ValueError):
        resolve_devices(bad, 8)


def test_devices_all_without_a_device_is_an_error():
    from pyorc_amd.executor import resolve_devices

    with pytest.raises(ValueError):
        resolve_devices("all", 0)


# ---- the cut of an in-memory stack -------------------------------------------------------------------------------------------------
def _plan_block(chunk_pairs):
    """A stand-in for the per-device chunk planner: chunks of ``chunk_pairs`` pairs over the block (relative frame slices)."""
    def plan(a, b, device, count):
        n = b - a
        return [(p, min(p + chunk_pairs, n) + 1) for p in range(0, n, chunk_pairs)]
    return plan


@pytest.mark.parametrize("n_pairs,D,align", [(200, 2, 25), (200, 3, 25), (401, 3, 25), (1000, 8, 75), (77, 2, 25), (31, 4, 1)])
def test_blocks_cover_every_pair_once_start_on_anchors_and_are_balanced(n_pairs, D, align):
    from pyorc_amd import velocimetry as V

    work = V.device_work(n_pairs + 1, None, [0] * D, align, False, _plan_block(2 * align))
    assert len(work) == D
    covered = []
    blocks = []
    for sl in work:
        pairs = [p for a, b in sl for p in range(a, b - 1)]
        covered += pairs
        for a, b in sl:
            assert a % align == 0                              # every chunk starts on an anchor of the absolute pair index
        if sl:
            blocks.append((sl[0][0], sl[-1][1] - 1))
            assert pairs == list(range(sl[0][0], sl[-1][1] - 1))   # contiguous
    assert covered == list(range(n_pairs))                     # every pair once, in device order
    units = [-(-(b - a) // align) for a, b in blocks]
    assert max(units) - min(units) <= 1                         # balanced to within one anchor


def test_more_devices_than_anchors_leaves_the_extra_devices_idle():
    from pyorc_amd import velocimetry as V

    work = V.device_work(51, None, [0, 0, 0, 0], 25, False, _plan_block(25))     # 50 pairs = 2 anchors
    assert sum(1 for sl in work if sl) == 2
    assert [p for sl in work for a, b in sl for p in range(a, b - 1)] == list(range(50))


def test_stack_signal_mode_hands_out_whole_chunks_of_the_single_device_plan():
    from pyorc_amd import velocimetry as V

    slices = V.aligned_slices(301, 51, 25)            # 300 pairs in chunks of 50
    work = V.device_work(301, slices, [0, 1, 2], 25, True, None)
    assert [s for sl in work for s in sl] == slices
    assert all(set(sl) <= set(slices) for sl in work)
    assert sorted(len(sl) for sl in work) == [2, 2, 2]
    few = V.device_work(301, slices[:2], [0, 1, 2, 3], 25, True, None)
    assert [len(sl) for sl in few].count(0) == 2 and [s for sl in few for s in sl] == slices[:2]


def test_no_devices_keeps_the_single_device_plan():
    from pyorc_amd import velocimetry as V

    slices = V.aligned_slices(201, 60, 25)
    assert V.device_work(201, slices, None, 25, False, None) == [slices]


def test_each_device_block_is_planned_against_its_share_of_that_devices_budget(monkeypatch):
    """Two workers on one device share its HBM: each block is planned against half of it."""
    from pyorc_amd import executor, velocimetry as V

    seen = []

    def plan_block(a, b, d, count):
        seen.append((d, count))
        return [(0, b - a + 1)]

    V.device_work(301, None, [0, 0, 1], 25, False, plan_block)
    assert seen == [(0, 2), (0, 2), (1, 1)]
    monkeypatch.setattr(executor, "bind_device", lambda d: None)
    monkeypatch.setattr(V.window, "available_memory", lambda: 16e9)
    monkeypatch.setattr(V.window, "chunk_alignment", lambda ws, dim=None, ov=None: 25)
    one = V._plan_slices(151, (1080, 1920), (32, 32), (16, 16), np.uint8, None, 1, "hip", 100, device=0, share=2)[2]
    small = V._plan_slices(151, (1080, 1920), (32, 32), (16, 16), np.uint8, 3, 1, "hip", 100, device=0, share=2)[2]
    assert one == [(0, 151)] and small[0] == (0, 26)


# ---- the lazy plan per device ------------------------------------------------------------------------------------------------------
def _lazy_plans(frames, devices, host=64e9, hbm=64e9, block_align=None):
    from pyorc_amd import velocimetry as V

    dim = tuple(frames[0].shape)
    n_rows, n_cols = V.window.get_array_shape(dim, (32, 32), (16, 16))
    return V.plan_lazy_devices(frames, len(frames), dim, (32, 32), (16, 16), n_rows * n_cols, None, 4, "hip", None, devices,
                               host_available=host, hbm_available=hbm)


def test_the_lazy_plan_divides_the_host_budget_and_gives_each_device_its_windows(monkeypatch):
    from pyorc_amd import executor
    from tests import lazy_doubles

    monkeypatch.delenv("LSPIV_PREFETCH_DEPTH", raising=False)
    monkeypatch.setattr(executor, "bind_device", lambda d: None)
    fr = lazy_doubles.from_frames(np.zeros((601, 96, 128), np.uint8), block=20)
    one = _lazy_plans(fr, None)
    three = _lazy_plans(fr, [0, 0, 0])
    assert len(one) == 1 and len(three) == 3
    for pl in three:
        assert pl["host_budget"] == pytest.approx(one[0]["host_budget"] / 3)
        assert pl["max_depth"] == max(1, one[0]["max_depth"] // 3)
    assert sum(pl["max_depth"] + 1 for pl in three) <= one[0]["max_depth"] + 1 + 3
    # one window set per device, each on its own frame range, the ranges joined by one shared (halo) frame
    ranges = [(pl["windows"][0][0], pl["windows"][-1][1]) for pl in three]
    assert ranges[0][0] == 0 and ranges[-1][1] == 601
    assert all(a[1] - 1 == b[0] for a, b in zip(ranges, ranges[1:]))
    for pl in three:
        w0 = pl["windows"][0][0]
        assert w0 % pl["align"] == 0 and w0 % 20 == 0          # on an anchor, and on dask's block boundary
        assert pl["loads"][0][0][0] == w0
    # too few common multiples of anchor and block for every device: cut on the anchors alone
    short = _lazy_plans(lazy_doubles.from_frames(np.zeros((201, 96, 128), np.uint8), block=20), [0, 0, 0])
    assert [pl["windows"][0][0] for pl in short] == [0, 50, 125]


def test_every_frame_is_loaded_once_but_the_boundary_frames(monkeypatch):
    """Counted through the loading double: the D - 1 halo frames are the only frames two devices load."""
    from pyorc_amd import executor, velocimetry as V
    from tests import lazy_doubles

    monkeypatch.setattr(executor, "bind_device", lambda d: None)
    T = 301
    fr = lazy_doubles.from_frames(np.zeros((T, 96, 128), np.uint8), block=20)
    for devices in ([0, 0], [0, 0, 0], [0, 1, 2, 3]):
        plans = _lazy_plans(fr, devices)
        counts = np.zeros(T, dtype=int)
        for pl in plans:
            for loads in pl["loads"]:
                for f0, f1 in loads:
                    piece = fr[f0:f1]
                    counts[f0:f1] += 1
                    assert len(V.load_frame_chunk(piece)) == f1 - f0
        twice = np.flatnonzero(counts == 2)
        active = sum(1 for pl in plans if pl is not None)
        assert len(twice) == active - 1 and counts.min() == 1 and counts.max() <= 2, (devices, twice)


def test_merged_stats_keep_todays_keys_and_add_the_devices():
    from pyorc_amd import velocimetry as V

    a = {"depth": 2, "workers": 4, "adaptive": True, "max_depth": 4, "depth_per_chunk": [1, 2], "chunks": 2, "load_s": 0.5,
         "waited_s": 0.25, "consumed_s": 1.0, "load_s_per_chunk": [0.25, 0.25], "waited_s_per_chunk": [0.2, 0.05]}
    b = dict(a, depth=3, chunks=1, depth_per_chunk=[3], load_s_per_chunk=[0.5], waited_s_per_chunk=[0.1])
    st = V._merge_stats([a, b, None], [0, 0, 0])
    assert set(a) <= set(st)
    assert st["chunks"] == 3 and st["depth"] == 3 and st["load_s"] == 1.0 and st["depth_per_chunk"] == [1, 2, 3]
    assert st["devices"] == [0, 0, 0] and len(st["per_device"]) == 3 and st["per_device"][2] == {} and st["idle_devices"] == 1
    one = V._merge_stats([a], None)
    assert {k: one[k] for k in a} == a and one["devices"] is None and one["per_device"] == [a]


# ---- the worker group ----------------------------------------------------------------------------------------------------------------
def test_the_first_worker_error_reaches_the_caller_and_no_thread_is_left(monkeypatch):
    import threading
    import time

    from pyorc_amd import executor

    monkeypatch.setattr(executor, "bind_device", lambda d: None)
    before = threading.active_count()

    def work(k, stop):
        if k == 1:
            raise RuntimeError("launch failed on worker 1")
        for _ in range(200):
            executor.stop_point(stop)
            time.sleep(0.01)
        return k

    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match="worker 1"):
        executor.run_on_devices([0, 0, 0], work)
    assert time.perf_counter() - t0 < 1.5
    assert threading.active_count() == before
    assert executor.run_on_devices([0, 0], lambda k, stop: k * 10) == [0, 10]
    assert executor.run_on_devices(None, lambda k, stop: "inline") == ["inline"]


# ---- the drop-in forwards the keyword ----------------------------------------------------------------------------------------------
def test_frames_get_piv_forwards_devices_to_get_ffpiv(monkeypatch):
    from pyorc_amd import _lib, plugin
    from tests import fake_xarray
    from tests.test_plugin import _fake_pyorc

    calls = []
    mods = _fake_pyorc(fake_xarray, calls)
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    monkeypatch.setitem(sys.modules, "xarray", fake_xarray)
    import pyorc_amd.velocimetry as V

    importlib.reload(V)
    plugin.uninstall()
    seen = {}

    def capture(frames, y, x, dt, *args, **kwargs):
        seen.update(kwargs)
        return fake_xarray.Dataset({}, coords={"y": y, "x": x})

    try:
        monkeypatch.setattr(V, "get_ffpiv", capture)
        monkeypatch.setattr(_lib, "require_device", lambda: None)
        fr = np.zeros((6, 96, 128), np.uint8)
        da = fake_xarray.DataArray(fr, ("time", "y", "x"), {"time": np.arange(6) / 25.0, "y": np.arange(96)[::-1] * 0.02,
                                                             "x": np.arange(128) * 0.02})
        assert plugin.install()
        mods["pyorc.api.frames"].Frames(da).get_piv(engine="hip", devices=[0, 0])
        assert seen["devices"] == [0, 0] and seen["engine"] == "hip"
        seen.clear()
        mods["pyorc.api.frames"].Frames(da).get_piv(engine="hip", devices="all")
        assert seen["devices"] == "all"
    finally:
        plugin.uninstall()
        monkeypatch.undo()
        importlib.reload(V)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_ensemble_allreduce_is_in_the_header_the_signatures_and_the_exports():
    from pyorc_amd import _lib

    header = open(os.path.join(ROOT, "include", "lspiv.h")).read()
    assert re.search(r"int\s+lspiv_ensemble_allreduce\s*\(\s*lspiv_ensemble\*\*\s*handles\s*,\s*int\s+n\s*\)\s*;", header)
    assert "lspiv_ensemble_allreduce" in _lib.SIGNATURES
    so = os.path.join(ROOT, "pyorc_amd", "liblspiv_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pyorc_amd", "csrc"), "-j8"])
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT lspiv_ensemble_allreduce$", syms, re.M)
    assert _lib.load().lspiv_abi_version() == 5


def test_the_allreduce_kernel_stays_out_of_the_kernel_hash_sources():
    from pyorc_amd import _lib

    for name in _lib.KERNEL_SOURCES:
        assert "allreduce" not in open(os.path.join(ROOT, "pyorc_amd", "csrc", name)).read()


# ---- the multi-worker assembly, end to end on the CPU ------------------------------------------------------------------------------
class _Lazy:
    """The least a lazy stack offers: ``load()`` and time slicing."""

    def __init__(self, data):
        self._d, self.dtype, self.shape = data, data.dtype, data.shape

    def __len__(self):
        return len(self._d)

    def __getitem__(self, key):
        return _Lazy(self._d[key]) if isinstance(key, slice) else self._d[key]

    def load(self):
        return np.array(self._d)


# LAST_STATS keys of today's runs: one worker keeps its own statistics (an ensemble's included), several are merged (no ``ensemble``;
# a lazy stack adds ``boundary_frames``)
_EAGER_KEYS = {"depth", "workers", "adaptive", "max_depth", "depth_per_chunk", "chunks", "load_s", "waited_s", "consumed_s",
               "load_s_per_chunk", "waited_s_per_chunk", "devices", "per_device", "idle_devices"}
_LAZY_KEYS = {"plan", "load_s", "waited_s", "upload_s", "launch_s", "chunks", "depth_per_chunk", "load_s_per_chunk", "waited_s_per_chunk",
              "depth", "workers", "adaptive", "devices", "per_device", "idle_devices"}


@pytest.mark.parametrize("ensemble", [False, True])
@pytest.mark.parametrize("lazy", [False, True])
def test_device_workers_assemble_the_single_worker_result(monkeypatch, lazy, ensemble):
    """``devices=[0, 0]`` and ``[0, 0, 0]`` against ``devices=None`` through the whole of ``get_ffpiv`` (oracle doubles for the launches):
    per-timestep results bit for bit, ensemble results to float32 rounding (the device-to-device sum is float32), and the statistics'
    keys as they are."""
    from pyorc_amd import _lib, executor, velocimetry as V
    from pyorc_amd.synth import particle_stack
    from tests import doubles
    from tests.test_shard_gloo import OracleEnsemble

    class Ens(OracleEnsemble):
        def accumulate(self, frames, corr_min, s2n_min, thr=None, out=None):
            return super().accumulate(np.asarray(frames), corr_min, s2n_min, thr, out)

        def close(self):
            pass

    def allreduce(handles):
        states = [h.export_state() for h in handles]
        s, k = states[0]
        for s1, k1 in states[1:]:
            s, k = s + s1, k + k1
        for h in handles:
            h.import_state(s, k)

    monkeypatch.setattr(executor, "bind_device", lambda d: None)
    monkeypatch.setattr(_lib, "device_count", lambda: 4)
    monkeypatch.setattr(V.piv, "piv_pairs", doubles.oracle_piv_pairs)
    monkeypatch.setattr(V.piv, "Ensemble", Ens)
    monkeypatch.setattr(V.piv, "ensemble_allreduce", allreduce)
    monkeypatch.setattr(V.window, "chunk_alignment", lambda ws, dim=None, ov=None: 5)
    monkeypatch.setattr(V.window, "available_memory", lambda: 1e12)
    doubles.use_host_stacks(monkeypatch)
    fr = particle_stack(33, 64, 96, seed=4).astype(np.float32)
    y, x = np.arange(3) * 0.5, np.arange(5) * 0.5
    dt = np.full(32, 0.04)

    def run(devices):
        ds = V.get_ffpiv(_Lazy(fr) if lazy else fr, y, x, dt, (32, 32), (16, 16), (32, 32), 0.02, 0.02, chunksize=11,
                         ensemble_corr=ensemble, devices=devices)
        return ds, dict(executor.LAST_STATS)

    ref, st = run(None)
    assert st["chunks"] >= 3                                   # several chunks (loads) per worker
    keys = _LAZY_KEYS if lazy else _EAGER_KEYS
    assert set(st) == keys | ({"ensemble"} if ensemble else set())
    for devices in ([0, 0], [0, 0, 0]):
        got, st = run(devices)
        assert set(st) == keys | ({"boundary_frames"} if lazy else set()), devices
        assert st["devices"] == devices and len(st["per_device"]) == len(devices) and st["idle_devices"] == 0
        assert np.array_equal(got.coords["time"], ref.coords["time"])
        for k in ("v_x", "v_y", "corr", "s2n"):
            if ensemble and k in ("v_x", "v_y"):
                np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-6, err_msg=f"{k} {devices}")
            else:
                assert np.array_equal(got[k], ref[k], equal_nan=True), (k, devices)
