"""Window deformation passes, host side (CPU): what the reference (tests/deform_ref.py) gains on sheared flow, the CPU checks of the
inputs tests/test_gpu_deform.py relies on (tie shares, signal fractions clear of the threshold), the keyword validation, the plugin's
TypeError for another engine, and the planner."""
import numpy as np
import pytest

from pyorc_amd import frames, piv, shard, velocimetry, window
from tests import deform_ref as ref
from tests import recipe_doubles as rd


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_reference_zero_nodes_warp_is_the_frame_and_the_plain_pass():
    from oracle import piv_oracle as po

    a = ref.pass_stack(16)
    n, ov, dim = ref.PASS_CASES[16]
    r = ref.pass_ref(16, nodes=None)
    assert np.array_equal(r["warped"], a[1:].astype(np.float64))
    _, _, oracle = po.cross_corr(a, (n, n), (ov, ov))
    assert np.array_equal(r["planes"], oracle)
    f = ref.pass_stack(16, np.float32)
    assert np.array_equal(ref.warp_stack(f, n, ov, np.zeros_like(ref.hand_nodes(16))), f[1:].astype(np.float64))


def test_reference_dense_field_hits_the_nodes_and_is_constant_outside():
    n, ov, dim = ref.PASS_CASES[32]
    nodes = ref.hand_nodes(32)[0].astype(np.int64)
    dv, du = ref.dense64(nodes, dim, n, ov)
    y0, x0 = ref.mp.grid_origins(dim, n, ov)
    # a node sits between the two central pixels of its window: the four of them average to it when their neighbours agree; on a constant
    # field every pixel carries the node rounded half up to 1 / 64 px
    const = np.broadcast_to(np.array([129, -257]), nodes.shape)
    cv, cu = ref.dense64(const, dim, n, ov)
    assert (cv == 65).all() and (cu == -128).all()                 # floor((129 + 1) / 2), floor((-257 + 1) / 2)
    assert (dv[:y0[0] + n // 2, :x0[0] + n // 2] == dv[0, 0]).all() and (du[y0[-1] + n // 2:, x0[-1] + n // 2:] == du[-1, -1]).all()
    assert dv[0, 0] == (nodes[0, 0, 0] + 1) // 2 and du[-1, -1] == (nodes[-1, -1, 1] + 1) // 2
    # one row of nodes: no interpolation along y
    n1, ov1, dim1 = ref.GRID_CASES["one-row"]
    dv1, _ = ref.dense64(ref.hand_nodes("one-row")[0], dim1, n1, ov1)
    assert (dv1 == dv1[0]).all()


def test_reference_predictor_rounds_to_even_and_skips_invalid():
    u = np.array([[[1 / 64 + 1 / 128, 3 / 64 + 1 / 128, np.nan]]], np.float32)      # q = 1.5 -> 2, 3.5 -> 4 (half to even)
    v = np.array([[[0.0, 0.0, 0.0]]], np.float32)
    m = ref.predict_nodes(u, v)
    assert m[0, 0, :, 1].tolist() == [2 + 4, 2 + 4, 2 * 4] and not m[..., 0].any()
    big = ref.predict_nodes(np.full((1, 1, 1), 3e38, np.float32), np.full((1, 1, 1), -1e9, np.float32))
    assert big[0, 0, 0].tolist() == [-2 * ref.QMAX, 2 * ref.QMAX]
    assert not ref.predict_nodes(np.full((1, 2, 2), np.nan, np.float32), np.zeros((1, 2, 2), np.float32)).any()


# ---- the value of the feature (the issue's figures: ratios 0.48 / 0.53, shares 0.68 / 0.67 against 0.16 / 0.20) ---------------------------
@pytest.mark.parametrize("seed", ref.ACCURACY_SEEDS)
def test_one_deformation_pass_halves_the_error_on_sheared_flow(seed):
    last, deformed = ref.accuracy_ref(seed)
    m0, s0 = ref.accuracy_figures(last["u"], last["v"])
    m1, s1 = ref.accuracy_figures(deformed["u"], deformed["v"])
    print(f"seed {seed}: integer chain median {m0:.4f} px, share <= 0.1 px {s0:.3f}; + one deformation pass {m1:.4f} px, {s1:.3f}; ratio {m1 / m0:.3f}")
    assert m1 <= 0.65 * m0
    assert s1 >= 0.55


# ---- the inputs the GPU tests rely on ---------------------------------------------------------------------------------------------------
def test_pass_inputs_have_rare_ties_and_nodes_that_cross_the_frame_edge():
    for case in list(ref.PASS_CASES) + list(ref.GRID_CASES):
        n, ov, (H, W) = ref.PASS_CASES[case] if case in ref.PASS_CASES else ref.GRID_CASES[case]
        nodes = ref.hand_nodes(case)
        for dtype in (ref.PASS_DTYPES if case in ref.PASS_CASES else (np.uint8,)):
            r = ref.pass_ref(case, dtype)
            print(case, dtype.__name__, "ties:", float(r["tie"].mean()), "finite:", float(np.isfinite(r["u"]).mean()))
            assert r["tie"].mean() <= 0.01, (case, dtype)
            assert np.isfinite(r["u"]).mean() > 0.5
        crossing = 0
        for p in range(nodes.shape[0]):
            dv, du = ref.dense64(nodes[p], (H, W), n, ov)
            Y, X = 64 * np.arange(H)[:, None] + dv, 64 * np.arange(W)[None, :] + du
            crossing += int(((Y < 0) | (Y > 64 * (H - 1)) | (X < 0) | (X > 64 * (W - 1))).sum())
        assert crossing > 0, case
        assert ref.pass_ref(case, nodes=None)["tie"].mean() <= 0.01
    for seed in ref.ACCURACY_SEEDS[:1]:
        assert all(r["tie"].mean() <= 0.01 for r in ref.accuracy_ref(seed))


def test_signal_inputs_are_clear_of_the_threshold():
    for case in ref.PASS_CASES:
        r = ref.signal_ref(case)
        fa, fb = ref.signal_fractions(case)
        assert not (np.abs(fa - ref.SIGNAL_THR) < 1e-6).any() and not (np.abs(fb - ref.SIGNAL_THR) < 1e-6).any(), case
        below = float(np.isnan(r["corr"]).mean())
        print(case, "below the threshold:", below, "ties:", float(r["tie"].mean()))
        assert 0.05 < below < 0.95 and r["tie"].mean() <= 0.01
        assert np.array_equal(np.isnan(r["corr"]), ~((fa >= ref.SIGNAL_THR) & (fb >= ref.SIGNAL_THR)).reshape(r["corr"].shape))


# ---- validation -------------------------------------------------------------------------------------------------------------------------
def test_deform_spec(lib):
    assert window.multipass_spec((32, 32), (16, 16), None, 0) == (32, 32) and window.multipass_spec((32, 32), (16, 16), [], None) == (32, 32)
    assert not isinstance(window.multipass_spec((32, 32), (16, 16), None, 0), window.MultiPassWindow)
    one = window.multipass_spec((32, 32), (16, 16), None, 2)
    assert isinstance(one, window.MultiPassWindow) and tuple(one) == (32, 32) and one.passes == ((32, 16),) and one.deform == 2
    spec = window.multipass_spec((32, 32), (16, 16), [64], np.int64(1))
    assert spec.passes == ((64, 32), (32, 16)) and spec.deform == 1 and window.multipass_spec(spec, (16, 16)) is spec
    assert window.multipass_spec((32, 32), (16, 16), [64]).deform == 0
    for d in (-1, 5, 1.0, "1", True):
        with pytest.raises(ValueError, match="deform_passes must be a whole number 0 .. 4"):
            window.multipass_spec((32, 32), (16, 16), None, d)
    for ws, ov in (((24, 24), (12, 12)), ((16, 32), (8, 8)), ((16, 16), (8, 4)), ((128, 128), (64, 64))):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            window.multipass_spec(ws, ov, None, 1)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        window.multipass_spec((24, 24), (12, 12), [64], 1)
    with pytest.raises(NotImplementedError, match="deform_passes together with a search_area_size"):
        window.multipass_spec(window.search_spec((12, 12), (32, 32)), (16, 16), None, 1)
    assert [lib.lspiv_deform_supported(n, n) for n in (8, 16, 24, 32, 48, 64, 128)] == [0, 1, 0, 1, 0, 1, 0]
    assert lib.lspiv_deform_supported(16, 32) == 0 and lib.lspiv_abi_version() == 5
    assert window.deform_supported((32, 32)) and not window.deform_supported((24, 24))


def test_keyword_validation():
    a = np.zeros((3, 96, 96), np.uint8)
    run = lambda ws=(16, 16), ov=(8, 8), sa=None, **kw: velocimetry.get_ffpiv(a, np.arange(3), np.arange(3), np.ones(2), ws, ov, sa or ws, 1.0, 1.0, **kw)
    for d in (-1, 5, 2.5):
        with pytest.raises(ValueError, match="deform_passes must be a whole number 0 .. 4"):
            run(deform_passes=d)
        with pytest.raises(ValueError, match="deform_passes must be a whole number 0 .. 4"):
            piv.piv_multipass(a, [(32, 16)], deform_passes=d)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        run((24, 24), (12, 12), deform_passes=1)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        frames.get_piv(a, 24, deform_passes=1)
    with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
        piv.piv_multipass(a, [(64, 32), (24, 12)], deform_passes=1)
    with pytest.raises(NotImplementedError, match="deform_passes with ensemble_corr=True is not implemented"):
        run(deform_passes=1, ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="deform_passes with ensemble_corr=True is not implemented"):
        run(deform_passes=1, coarse_passes=[64], ensemble_corr=True)
    with pytest.raises(NotImplementedError, match="deform_passes together with a search_area_size"):
        run((12, 12), (16, 16), (32, 32), deform_passes=1)

    class Comm:
        rank, world = 0, 1

    spec = window.multipass_spec((16, 16), (8, 8), None, 1)
    with pytest.raises(NotImplementedError, match="deform_passes with pyorc_amd.shard is not implemented"):
        shard.sharded_piv(lambda f0, f1: a[f0:f1], 2, spec, (8, 8), Comm())
    with pytest.raises(NotImplementedError, match="with pyorc_amd.shard is not implemented"):
        shard.sharded_piv_dev(object(), 2, window.multipass_spec((16, 16), (8, 8), [64], 1), (8, 8), Comm())


def test_other_engines_do_not_know_the_keyword(monkeypatch):
    from pyorc_amd import plugin

    rd.install(monkeypatch.setitem)
    try:
        acc = rd.Frames(np.zeros((3, 96, 96), np.uint8))
        with pytest.raises(TypeError, match="deform_passes is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", deform_passes=1)
        with pytest.raises(TypeError, match="deform_passes is a keyword of engine='hip' only"):
            acc.get_piv(16, engine="numba", deform_passes=0)
    finally:
        plugin.uninstall()


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def test_planner_adds_one_batch_of_warped_frames_and_the_nodes(lib):
    dim, T = (160, 200), 10
    spec = window.multipass_spec((32, 32), (16, 16), [64], 1)
    plain = window.required_memory(T, dim, (32, 32), (16, 16), coarse_passes=[64])
    need = window.required_memory(T, dim, (32, 32), (16, 16), coarse_passes=[64], deform_passes=1)
    assert need == window.required_memory(T, dim, spec, (16, 16)) == window.required_memory(T, dim, (32, 32), (16, 16), coarse_passes=[64], deform_passes=3)
    n_win = int(np.prod(window.get_array_shape(dim, (32, 32), (16, 16))))
    assert need - plain == (T - 1) * 160 * 200 * 4 + (T - 1) * n_win * 8 == window.deform_bytes(T, dim, (32, 32), (16, 16))
    assert window.required_memory(T, dim, (32, 32), (16, 16), coarse_passes=[64], deform_passes=0) == plain
    # without coarse passes: the plain call plus the same terms
    alone = window.required_memory(T, dim, (32, 32), (16, 16), deform_passes=1)
    assert alone == window.required_memory(T, dim, (32, 32), (16, 16)) + window.deform_bytes(T, dim, (32, 32), (16, 16))
    # the warped frames are those of ONE batch: at most 256 MiB (one frame at least), however many pairs
    big = window.deform_bytes(2001, (1080, 1920), (32, 32), (16, 16))
    n_big = int(np.prod(window.get_array_shape((1080, 1920), (32, 32), (16, 16))))
    assert big == ((256 << 20) // (1080 * 1920 * 4)) * 1080 * 1920 * 4 + 2000 * n_big * 8
    assert window.deform_bytes(3, (20000, 20000), (64, 64), (32, 32)) - 2 * int(np.prod(window.get_array_shape((20000, 20000), (64, 64), (32, 32)))) * 8 \
        == 20000 * 20000 * 4
    assert window.chunk_alignment(window.multipass_spec((32, 32), (16, 16), None, 1), dim, (16, 16)) == window.chunk_alignment((32, 32), dim, (16, 16))


# ---- the inputs of tests/test_gpu_rescue_modes.py and tests/test_gpu_batch_loops.py ---------------------------------------------------------
@pytest.mark.parametrize("n,ov", ref.mp.RESCUE_GEOMETRIES, ids=[f"{n}@{ov}" for n, ov in ref.mp.RESCUE_GEOMETRIES])
def test_rescue_inputs_have_no_ties(n, ov):
    """Measured: tie share 0.0 for both node fields at every geometry and sample type; finite windows 94.5 % / 94.3 % (uniform / mixed) at
    16 @ 8, 100 % / 93.5 % at 32 @ 16, all of them at 64 @ 32 and 64 @ 48."""
    for field in ref.RESCUE_FIELDS:
        for dtype in ref.PASS_DTYPES:
            r = ref.rescue_ref(n, ov, field, dtype)
            print(n, ov, field, dtype.__name__, "ties:", float(r["tie"].mean()), "finite:", float(np.isfinite(r["u"]).mean()))
            assert r["tie"].mean() <= 0.01 and np.isfinite(r["u"]).mean() >= 0.93
    uniform, mixed = (ref.rescue_nodes(n, ov, f) for f in ref.RESCUE_FIELDS)
    assert (uniform[..., 1] == 128).all() and not uniform[..., 0].any()
    assert {tuple(q) for q in mixed.reshape(-1, 2)} == {(0, 128), (0, 64), (-37, 128), (-37, 64)}
    # the uniform field is a whole-pixel move of frame t+1: the warp interpolates nothing
    a = ref.mp.rescue_stack()
    assert np.array_equal(ref.rescue_ref(n, ov, "uniform")["warped"][:, :, :-1], a[1:, :, 1:].astype(np.float64))


def test_batch_workspaces_of_one_and_two_frames_cut_the_pass_cases_into_batches(lib):
    """LSPIV_DEFORM_WS_BYTES, as tests/test_gpu_batch_loops.py sets it: lspiv_deform_required_bytes reports the batch it gives."""
    import os
    from unittest import mock

    for case, (n, ov, (H, W)) in ref.PASS_CASES.items():
        n_win = int(np.prod(window.get_array_shape((H, W), (n, n), (ov, ov))))
        nodes = (ref.PASS_T - 1) * n_win * 8
        frame = H * W * 4
        assert lib.lspiv_deform_required_bytes(ref.PASS_T, H, W, n, n, ov, ov) == 3 * frame + nodes          # unset: one batch
        for env, batch in ((frame, 1), (2 * frame, 2), (2 * frame - 1, 1), (1, 1), (0, 1), (3 * frame, 3), (1 << 40, 3)):
            with mock.patch.dict(os.environ, {"LSPIV_DEFORM_WS_BYTES": str(env)}):
                assert lib.lspiv_deform_required_bytes(ref.PASS_T, H, W, n, n, ov, ov) == batch * frame + nodes, (case, env)
        assert lib.lspiv_deform_required_bytes(ref.PASS_T, H, W, n, n, ov, ov) == 3 * frame + nodes
