"""The recipe's frame filters inside the pyorc drop-in, host side (CPU): ``install()`` records ``Frames.normalize`` / ``edge_detect`` /
``minmax`` / ``smooth`` results, ``hip_projection_source`` resolves a chain of them under ``project_hip``, ``plan_lazy`` budgets its
scratch, and ``get_ffpiv`` loads the uint8 camera blocks and runs the chain instead of the host filters (doubles: tests/recipe_doubles.py,
the chain computed by the oracle on host stacks)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import recipe_doubles as rd  # noqa: E402

SRC, DST = (96, 128), (72, 100)


@pytest.fixture
def dropin(monkeypatch):
    """The pyorc double installed, xarray's double in place, no GPU: projection, PIV and HBM stacks by their oracles."""
    from pyorc_amd import _lib, plugin, project as P, velocimetry as V
    from tests import doubles, lazy_doubles
    from tests.test_round6_host import OraclePlan

    monkeypatch.setitem(sys.modules, "xarray", lazy_doubles)
    monkeypatch.setattr(P, "Projection", OraclePlan)
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(V.piv, "piv_pairs", doubles.oracle_piv_pairs)
    monkeypatch.setattr(V.window, "available_memory", lambda: 1e12)
    monkeypatch.setattr(V.window, "chunk_alignment", lambda ws, dim=None, ov=None: 10)
    OraclePlan.made = []
    rd.Frames.made = []
    rd.install(monkeypatch.setitem)
    yield rd.Frames
    plugin.uninstall()


def _maps():
    from pyorc_amd.synth import projection_maps

    return projection_maps(SRC, DST, tilt=0.2, seed=4)


def _cam(T=47):
    from pyorc_amd.synth import particle_stack

    return particle_stack(T, SRC[0], SRC[1], seed=12)


def _project(stack):
    from pyorc_amd import plugin
    from tests import lazy_doubles

    return lazy_doubles.frames_project(stack, _maps(), DST, plugin.project_hip)


def _recipe(Fr, root):
    return Fr(Fr(Fr(root).normalize(15)).edge_detect(1, 2)).minmax(-5, 5)


def test_install_wraps_the_filters_and_uninstall_restores_them(monkeypatch):
    from pyorc_amd import plugin

    plugin.uninstall()
    orig = {op: rd.Frames.__dict__[op] for op in ("normalize", "edge_detect", "minmax", "smooth", "time_diff", "get_piv")}
    rd.install(monkeypatch.setitem)
    try:
        for op in ("normalize", "edge_detect", "minmax", "smooth"):
            assert rd.Frames.__dict__[op] is not orig[op] and rd.Frames.__dict__[op].__lspiv_original__ is orig[op], op
        assert rd.Frames.__dict__["time_diff"] is orig["time_diff"]          # not wrapped in this issue
        root = rd.camera(_cam(), block=10)
        rd.Frames.made = []
        for call in (lambda: rd.Frames(root).normalize(15), lambda: rd.Frames(root).edge_detect(1, 2),
                     lambda: rd.Frames(rd.Frames(root).smooth(2)).minmax(0, 100)):
            out = call()
            assert out is rd.Frames.made[-1]                                 # the original's object, unchanged
        names = dict(plugin._FILTERS)
        assert {v[0] for v in names.values()} == {"normalize", "edge_detect", "smooth", "minmax"}
        assert names[rd.Frames.made[-1].data.name] == ("minmax", {"min": 0.0, "max": 100.0}, rd.Frames.made[-2])
        assert names[rd.Frames.made[0].data.name] == ("normalize", {"samples": 15}, root)
        assert names[rd.Frames.made[1].data.name][1] == {"wdw_1": 1, "wdw_2": 2}
        # an eager result (no dask name) is not recorded; a kernel size the device chain cannot run is not either
        eager = rd.Frames(np.zeros((4, 8, 8), np.uint8))
        n = len(plugin._FILTERS)
        assert plugin._wrap_filter("minmax", lambda self, min=-np.inf, max=np.inf: np.zeros(3))(eager) is not None
        assert len(plugin._FILTERS) == n
        rd.Frames(root).edge_detect(1, 16)                                    # 33 x 33
        assert len(plugin._FILTERS) == n
    finally:
        plugin.uninstall()
    for op, fn in orig.items():
        assert rd.Frames.__dict__[op] is fn, op
    assert plugin._FILTERS == {}


def test_the_recipe_chain_resolves_to_its_uint8_root(dropin):
    from pyorc_amd import plugin

    root = rd.camera(_cam(), block=10)
    ortho = _project(_recipe(dropin, root))
    hit = plugin.hip_projection_source(ortho)
    assert hit is not None and hit["root"] is root and hit["source"] is dropin.made[-1] and hit["dst_shape"] == DST
    assert hit["ops"] == [("normalize", {"samples": 15}), ("edge_detect", {"wdw_1": 1, "wdw_2": 2}), ("minmax", {"min": -5.0, "max": 5.0})]
    # an unregistered layer BELOW the ops is the root: the host computes it, the chain starts above it
    decoded = rd.camera(_cam(), block=10, layer="decode")
    hit = plugin.hip_projection_source(_project(dropin(dropin(decoded).smooth(1)).minmax(0, 200)))
    assert hit["root"] is decoded and [op for op, _ in hit["ops"]] == ["smooth", "minmax"]


def test_anything_else_resolves_to_todays_answer(dropin):
    from pyorc_amd import plugin

    root = rd.camera(_cam(), block=10)
    Fr = dropin
    cases = {}
    mm = _recipe(Fr, root)
    extra = mm.map_time(lambda blk: blk, "astype")                         # a layer between the last filter and project_hip
    cases["extra layer"] = (_project(extra), extra)
    td = Fr(Fr(Fr(Fr(root).normalize(15)).time_diff()).edge_detect(1, 2)).minmax(-5, 5)   # time_diff (not wrapped) above the root
    cases["time_diff"] = (_project(td), td)
    flt = rd.camera(_cam().astype(np.float32), block=10)                   # a float root
    e = Fr(flt).edge_detect(1, 2)
    cases["float root"] = (_project(e), e)
    m8 = Fr(root).minmax(0, 100)                                           # minmax straight on uint8
    cases["minmax on uint8"] = (_project(m8), m8)
    two = Fr(Fr(root).smooth(1)).edge_detect(1, 2)                         # two Gaussian stages: one float scratch stack per piece
    cases["two blurs"] = (_project(two), two)
    late = Fr(Fr(root).edge_detect(1, 2)).normalize(15)                    # normalize not first
    cases["normalize late"] = (_project(late), late)
    for what, (ortho, source) in cases.items():
        hit = plugin.hip_projection_source(ortho)
        assert hit is not None and "ops" not in hit and "root" not in hit and hit["source"] is source, what   # today's hand-off
    # filters applied after project: not project_hip's product -- None, as today
    after = Fr(_project(root)).edge_detect(1, 2)
    assert plugin.hip_projection_source(after) is None


def test_the_chain_scratch_is_budgeted_per_loader(dropin):
    from pyorc_amd import executor, velocimetry as V, window

    root = rd.camera(_cam(201), block=20)
    n_rows, n_cols = window.get_array_shape(DST, (32, 32), (16, 16))
    px = SRC[0] * SRC[1]

    def plan(stack):
        return V.plan_lazy(_project(stack), 201, DST, (32, 32), (16, 16), n_rows * n_cols, None, 4, "hip", None, host_available=64e9,
                           hbm_available=1e12)

    p = plan(_recipe(dropin, root))
    deepest = executor.max_depth()
    assert p["source"] == "camera" and p["chain"].names == ["normalize", "edge_detect", "minmax"]
    assert p["host_frame_bytes"] == px                                       # host loads counted in uint8 root bytes
    assert p["hbm_scratch"] == (deepest + 1) * p["load_frames"] * (1 + 1 + 4) * px + 4 * px
    p = plan(dropin(root).edge_detect(2, 3))
    assert p["hbm_scratch"] == (deepest + 1) * p["load_frames"] * (1 + 4) * px
    p = plan(dropin(root).normalize(15))
    assert p["hbm_scratch"] == (deepest + 1) * p["load_frames"] * (1 + 1) * px + 4 * px
    # today's hand-off keeps today's term: one load of the camera frames it loads
    extra = _recipe(dropin, root).map_time(lambda blk: blk, "astype")
    p = plan(extra)
    assert p["chain"] is None and p["host_frame_bytes"] == 4 * px and p["hbm_scratch"] == p["load_frames"] * 4 * px


@pytest.mark.parametrize("ensemble", [False, True])
def test_the_dropin_runs_the_chain_instead_of_the_host_filters(dropin, monkeypatch, ensemble):
    """The recipe under project_hip: no block of the double's filter layers is computed, uint8 camera blocks are loaded and handed to the
    chain, LAST_STATS reports it -- and the bits are those of the host filters feeding today's hand-off."""
    from pyorc_amd import executor, frames as F, plugin
    from tests import doubles

    if ensemble:
        from tests.test_shard_gloo import OracleEnsemble
        from pyorc_amd import velocimetry as V

        class Ens(OracleEnsemble):
            def accumulate(self, frames, corr_min, s2n_min, thr=None, out=None):
                return super().accumulate(np.asarray(frames), corr_min, s2n_min, thr, out)

            def finish(self, count_min, n_frames):
                mean = self.s / np.maximum(self.k, 1)[:, None, None]
                u, v = self.po.u_v_displacement(mean[None], self.n_rows, self.n_cols)
                return u.astype(np.float32), v.astype(np.float32), self.k.astype(np.float32)

            def close(self):
                pass

        monkeypatch.setattr(V.piv, "Ensemble", Ens)
    stacks = doubles.use_host_stacks(monkeypatch)
    seen = []
    rd.host_chain(monkeypatch, seen)
    cam = _cam()
    t = np.arange(47) / 30.0
    kw = dict(time=t, resolution=0.01, ensemble_corr=ensemble)
    root = rd.camera(cam, block=10, layer="decode")
    mm = _recipe(dropin, root)
    got = F.get_piv(_project(mm), 32, **kw)
    st = dict(executor.LAST_STATS)
    assert st["plan"]["source"] == "camera" and st["plan"]["chain"] == ["normalize", "edge_detect", "minmax"]
    assert rd.filter_blocks(mm) == {}                                       # not one block of the host filters
    assert seen and all(dt == np.uint8 for dt in seen) and len(seen) == st["chunks"]   # the uint8 camera blocks went up
    assert stacks.uploads == []
    # today's path on the same graph: the host filters feed the hand-off
    plugin._FILTERS.clear()
    ref = F.get_piv(_project(mm), 32, **kw)
    assert "chain" not in executor.LAST_STATS["plan"] and executor.LAST_STATS["plan"]["source"] == "camera"
    assert rd.filter_blocks(mm) == {(layer, i): 1 for layer in ("normalize", "edge_detect", "minmax") for i in range(5)}
    for k in ("v_x", "v_y", "corr", "s2n"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
