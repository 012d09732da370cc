"""The recipe's frame filters inside the pyorc drop-in, on the MI355X: ``normalize -> edge_detect -> minmax`` (or ``smooth``) ahead of
``project(method="hip")`` and ``get_piv(engine="hip")`` run on the device (uint8 camera blocks uploaded, ``filters.Chain`` in the resident
stack's staging), bit-equal to today's hand-off fed with the device mirrors' output of the same filters.  Doubles: tests/recipe_doubles.py
(pyorc's Frames, with the filters of oracle/filters_oracle.py as counted per-block layers) over tests/lazy_doubles.py."""
import sys
import warnings

import numpy as np
import pytest

from pyorc_amd.synth import particle_stack, projection_maps
from tests import recipe_doubles as rd

pytestmark = pytest.mark.gpu

SRC, DST = (270, 480), (200, 360)
T = 91


@pytest.fixture
def dropin(gpu, monkeypatch):
    from pyorc_amd import plugin
    from tests import lazy_doubles

    monkeypatch.setitem(sys.modules, "xarray", lazy_doubles)
    rd.Frames.made = []
    rd.install(monkeypatch.setitem)
    yield rd.Frames
    plugin.uninstall()


def _maps():
    return projection_maps(SRC, DST, tilt=0.1, seed=2)


def _project(stack):
    from pyorc_amd import plugin
    from tests import lazy_doubles

    return lazy_doubles.frames_project(stack, _maps(), DST, plugin.project_hip)


def _kw(n, **extra):
    return dict(time=np.arange(n) / 30.0, resolution=0.01, **extra)


def _reference(filtered, block, **kw):
    """R: today's hand-off over a lazy stack whose blocks are the device mirrors' output (the float32 camera frames are loaded, uploaded
    and projected into the resident stack)."""
    from pyorc_amd import executor, frames as F
    from tests import lazy_doubles

    r = F.get_piv(_project(lazy_doubles.from_frames(filtered, block=block)), 32, **kw)
    assert executor.LAST_STATS["plan"]["source"] == "camera" and "chain" not in executor.LAST_STATS["plan"]
    return r


def _equal(got, ref, what):
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)


def _recipe(Fr, root):
    return Fr(Fr(Fr(root).normalize(15)).edge_detect(1, 2)).minmax(-5, 5)


def _mirror_recipe(cam):
    from pyorc_amd import filters

    return filters.minmax(filters.edge_detect(filters.normalize(cam, 15), 1, 2), -5, 5)


CASES = {
    "recipe": (_recipe, _mirror_recipe, ["normalize", "edge_detect", "minmax"]),
    # 13 x 13 and 21 x 21: the blur kernel with a run-time radius
    "edge_detect(6, 10) on raw uint8": (lambda Fr, root: Fr(root).edge_detect(6, 10), lambda cam: _mirror_edge(cam), ["edge_detect"]),
    "normalize -> smooth -> minmax": (lambda Fr, root: Fr(Fr(Fr(root).normalize(15)).smooth(1)).minmax(0, 200),
                                      lambda cam: _mirror_smooth(cam), ["normalize", "smooth", "minmax"]),
}


def _mirror_edge(cam):
    from pyorc_amd import filters

    return filters.edge_detect(cam, 6, 10)


def _mirror_smooth(cam):
    from pyorc_amd import filters

    return filters.minmax(filters.smooth(filters.normalize(cam, 15), 1), 0, 200)


@pytest.mark.parametrize("case,block,extra", [("recipe", 20, {}), ("edge_detect(6, 10) on raw uint8", 20, {}),
                                              ("normalize -> smooth -> minmax", 20, {}), ("recipe", 7, {"chunksize": 10}),
                                              ("recipe", 20, {"ensemble_corr": True})])
def test_the_chain_dropin_is_bit_equal_to_todays_handoff(dropin, case, block, extra):
    from pyorc_amd import executor, frames as F

    chain, mirror, names = CASES[case]
    cam = particle_stack(T, SRC[0], SRC[1], seed=8)
    kw = _kw(T, **extra)
    ref = _reference(mirror(cam), block, **kw)
    stack = chain(dropin, rd.camera(cam, block=block))
    got = F.get_piv(_project(stack), 32, **kw)
    st = dict(executor.LAST_STATS)
    assert st["plan"]["source"] == "camera" and st["plan"]["chain"] == names, st["plan"]
    assert rd.filter_blocks(stack) == {}                                     # the host filters never ran
    if block == 7:
        assert st["plan"]["load_frames"] == 10 and st["chunks"] == -(-T // 7)     # loads cut on the 7-frame blocks
    _equal(got, ref, case)


def test_a_small_hbm_budget_splits_the_chain_run_into_windows(dropin, monkeypatch):
    from pyorc_amd import executor, frames as F, velocimetry as V

    cam = particle_stack(T, SRC[0], SRC[1], seed=8)
    ref = _reference(_mirror_recipe(cam), 20, **_kw(T))
    monkeypatch.setattr(V.window, "available_memory", lambda: 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the reference's "Memory availability is poor" of get_ffpiv's chunk planner
        got = F.get_piv(_project(_recipe(dropin, rd.camera(cam))), 32, **_kw(T))
    st = dict(executor.LAST_STATS)
    assert st["plan"]["chain"] == ["normalize", "edge_detect", "minmax"] and len(st["plan"]["windows"]) > 1, st["plan"]
    _equal(got, ref, "windows")


@pytest.mark.parametrize("case", ["time_diff", "extra layer"])
def test_what_is_not_a_chain_keeps_todays_path(dropin, case):
    from pyorc_amd import executor, frames as F, plugin

    cam = particle_stack(T, SRC[0], SRC[1], seed=8)
    Fr = dropin
    root = rd.camera(cam)
    if case == "time_diff":
        stack = Fr(Fr(Fr(Fr(root).normalize(15)).time_diff()).edge_detect(1, 2)).minmax(-5, 5)
    else:
        stack = _recipe(Fr, root).map_time(lambda blk: blk, "astype")
    n = len(stack)
    ortho = _project(stack)
    got = F.get_piv(ortho, 32, **_kw(n))
    assert "chain" not in executor.LAST_STATS["plan"] and executor.LAST_STATS["plan"]["source"] == "camera"
    ran = rd.filter_blocks(stack, ("edge_detect", "minmax"))
    assert ran and all(v == 1 for v in ran.values())                        # the host filters ran, each block once
    plugin._FILTERS.clear()                                                 # today: nothing recorded
    ref = F.get_piv(ortho, 32, **_kw(n))
    _equal(got, ref, case)
