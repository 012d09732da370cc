"""GPU tests of pyramidal Lucas-Kanade point tracking against tests/track_ref.py, on the inputs that
tests/test_track_host.py qualified: the pyramid bit for bit; the tracker with fixed iteration counts (unconverged states, where any
arithmetic slip shows) and converged, with status and n_iter equal on every point and u, v within 1e-9 px; the same bits from run to
run, from the host twin and DeviceFrames, from time slices, from workspace batches, and from trajectories against one-pair calls.
Every one of the 28 (window, dtype) instances of the kernel runs against the reference in four modes and, against the reference summed
in the kernel's order, bit for bit in two (ti.VARIANT_CASES); so do scenes with a NaN, +inf or -inf sample and guesses beyond the index
clamp; five levels go through the batch, chunk and chain loops."""

import numpy as np
import pytest

from pyorc_amd import DeviceFrames, _lib, track
from tests import track_inputs as ti
from tests import track_ref as tr

pytestmark = pytest.mark.gpu

GATE_D = 1e-9          # px: the gate of the stabilise fit, four orders above what the order of the float64 sums explains (7e-16)
GATE_REL = 1e-9        # err relative to sum |I| / w^2, min_eig relative to (Gxx + Gyy) / w^2
FIELDS = ("u", "v", "status", "err", "min_eig", "n_iter")


def _same_bits(got, want):
    """Equal bit for bit (the sign of a zero included); a NaN must be a NaN (its payload is the hardware's own)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    kind = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(kind)[~nan], want.view(kind)[~nan])


def _same_tracks(a, b):
    return all(_same_bits(getattr(a, n), getattr(b, n)) for n in FIELDS)


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------
def _pyr_frames(dtype, T, shape, special):
    rng = np.random.default_rng(T * 1000 + shape[0] * 7 + shape[1])
    f = rng.integers(0, 256, size=(T,) + shape)
    if dtype == np.uint8:
        return f.astype(np.uint8)
    f = (f + rng.random(f.shape) - 100.0).astype(np.float32)
    if special:
        kind = rng.random(f.shape)
        f[kind < 0.03] = np.nan
        f[(kind >= 0.03) & (kind < 0.12)] = 0.0
        f[(kind >= 0.12) & (kind < 0.21)] = -0.0
    return f


@pytest.mark.parametrize("shape", [(3, 3), (4, 5), (33, 47), (48, 64), (70, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", ["uint8", "float32", "float32-nan-zeros"])
def test_pyr_down_is_the_references_bits(gpu, case, shape):
    dtype = np.uint8 if case == "uint8" else np.float32
    for T in (2, 3, 5):
        f = _pyr_frames(dtype, T, shape, case.endswith("zeros"))
        want = tr.pyr_down(f)
        got = track.pyr_down(f)
        assert got.shape == (T, (shape[0] + 1) // 2, (shape[1] + 1) // 2) and _same_bits(got, want)
        dev = track.pyr_down(DeviceFrames.from_host(f))
        assert isinstance(dev, DeviceFrames) and _same_bits(dev.to_host(), want)
    if min(shape) >= 5:      # the second level from the first, float32 -> float32
        assert _same_bits(track.pyr_down(got), tr.pyr_down(want))


# ---- the tracker against the reference ------------------------------------------------------------------------------------------------------
def _check_against_reference(got, ref, case, what):
    assert np.array_equal(got.status, ref["status"]), f"{what}: status differs on {(got.status != ref['status']).sum()} points"
    assert np.array_equal(got.n_iter, ref["n_iter"]), f"{what}: n_iter differs on {(got.n_iter != ref['n_iter']).sum()} points"
    worst = {}
    # u, v in px; err relative to sum |I| / w^2 and min_eig relative to (Gxx + Gyy) / w^2 of the point's own template
    for name, gate, scale in (("u", GATE_D, 1.0), ("v", GATE_D, 1.0), ("err", GATE_REL, ref["err_scale"]), ("min_eig", GATE_REL, ref["eig_scale"])):
        g, r = getattr(got, name), ref[name]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN of {name} is not where the reference has it"
        with np.errstate(invalid="ignore", divide="ignore"):
            off = np.abs(g - r) / scale
        off = off[np.isfinite(r) & (g != r)]            # (equal values need no scale: a flat template has min_eig = 0 over a scale of 0)
        worst[name] = float(off.max()) if off.size else 0.0
        assert worst[name] <= gate, f"{what}: {name} off by {worst[name]:.3e} > {gate:.1e}"
    lost = ref["status"] >= 2
    assert np.isnan(got.u[lost]).all() and np.isnan(got.v[lost]).all() and np.isnan(got.err[lost]).all()
    assert got.status.dtype == np.uint8 and got.n_iter.dtype == np.int32
    return worst


@pytest.mark.parametrize("case", ti.CASES, ids=ti.case_id)
def test_fixed_iterations_are_the_references(gpu, case):
    shape, kind, T, N, w, L = case
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    for mode in ("fixed1", "fixed2", "fixed5"):
        got = track.track_pairs(f, p, **ti.kwargs(case, mode))
        worst = _check_against_reference(got, ti.reference(case, mode), case, mode)
        print(ti.case_id(case), mode, "largest difference:", ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        alive = got.status < 2
        assert (got.status[alive] == 1).all()                       # eps = 0: no level ever converges
        assert (got.n_iter[alive] == L * ti.MODES[mode]["max_iter"]).all()


@pytest.mark.parametrize("case", ti.CASES, ids=ti.case_id)
def test_converged_tracks_are_the_references(gpu, case):
    shape, kind, T, N, w, L = case
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    for mode in ("converge", "converge-min-eig", "converge-guess"):
        got = track.track_pairs(f, p, **ti.kwargs(case, mode))
        worst = _check_against_reference(got, ti.reference(case, mode), case, mode)
        print(ti.case_id(case), mode, "largest difference:", ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_the_kernels_sums_are_the_lane_trees_bits(gpu):
    """With the reference's sums in the kernel's order nothing is left to differ: the same bits."""
    for case in (ti.CASES[2], ti.CASES[5]):       # template in registers (w = 15) and in the patch (w = 31)
        shape, kind, T, N, w, L = case
        got = track.track_pairs(ti.scene(shape, T, kind), ti.points(shape, N), **ti.kwargs(case, "fixed2"))
        ref = ti.reference(case, "fixed2", "lanes")
        assert all(_same_bits(getattr(got, n), ref[n]) for n in FIELDS)


# ---- every instance of the kernel: ti.VARIANT_CASES, one (window, dtype) per id ------------------------------------------------------------
def _run(case, mode):
    shape, kind, T, N, w, L = case
    return track.track_pairs(ti.scene(shape, T, kind), ti.points(shape, N), **ti.kwargs(case, mode))


def _parity(case, modes):
    """Every mode against the float64 reference; eps = 0: no level ever converges, so every level runs max_iter iterations."""
    family = "registers" if case[4] <= ti.REG_WINDOW else "patch"
    for mode in modes:
        got, ref = _run(case, mode), ti.reference(case, mode)
        worst = _check_against_reference(got, ref, case, mode)
        print(ti.case_id(case), mode, f"({family})", "largest difference:", ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        for lost in (tr.STATUS_OUT, tr.STATUS_NOT_FINITE):
            assert (got.status[ref["status"] == lost] == lost).all()
        if mode == "fixed2":
            alive = got.status < 2
            assert (got.status[alive] == 1).all() and (got.n_iter[alive] == case[5] * 2).all()


def _lane_bits(case, modes):
    """With the reference's sums in the kernel's order nothing is left to differ: the same bits in every field."""
    for mode in modes:
        got, ref = _run(case, mode), ti.reference(case, mode, "lanes")
        for n in FIELDS:
            assert _same_bits(getattr(got, n), ref[n]), (mode, n)


@pytest.mark.parametrize("case", ti.VARIANT_CASES, ids=ti.case_id)
def test_every_instance_is_the_references(gpu, case):
    _parity(case, ti.VARIANT_MODES)


@pytest.mark.parametrize("case", ti.VARIANT_CASES, ids=ti.case_id)
def test_every_instances_sums_are_the_lane_trees_bits(gpu, case):
    _lane_bits(case, ti.LANE_MODES)


@pytest.mark.parametrize("case", ti.NOT_FINITE_CASES, ids=ti.case_id)
def test_a_sample_that_is_not_finite_is_status_4_where_the_reference_has_it(gpu, case):
    _parity(case, ti.VARIANT_MODES)
    _lane_bits(case, ti.LANE_MODES)
    got = _run(case, "converge")
    assert (got.status == tr.STATUS_NOT_FINITE).any(axis=1).all()       # in pair 0 (the sample is in J) and in pair 1 (in the template)
    assert np.isnan(got.u[got.status == tr.STATUS_NOT_FINITE]).all()


@pytest.mark.parametrize("case", ti.FAR_CASES, ids=ti.case_id)
def test_a_guess_beyond_the_index_clamp_walks_out_after_one_iteration(gpu, case):
    """Guesses of 1e12 and -3e9 px: split() clamps the position at +-2^30 and bilinear() the indices to the level, as the reference does."""
    _parity(case, ("far-guess",))
    _lane_bits(case, ("far-guess",))
    got = _run(case, "far-guess")
    far = sorted(ti.FAR_POINTS)
    assert (got.status[:, far] == tr.STATUS_OUT).all() and (got.n_iter[:, far] == 1).all() and np.isnan(got.u[:, far]).all()


def test_a_point_that_is_not_finite_has_status_5_through_the_c_abi(gpu):
    shape, T, N = (33, 47), 3, 5
    f = ti.scene(shape, T, "uint8")
    p = np.ascontiguousarray(ti.points(shape, N).copy())
    p[1, 0] = np.nan
    p[4, 1] = np.inf
    out = [np.zeros((T - 1, N)) for _ in range(4)]
    n_iter, status = np.zeros((T - 1, N), dtype=np.int32), np.zeros((T - 1, N), dtype=np.uint8)
    _lib.check(gpu.lspiv_lk_track(_lib.ptr(f), 0, T, *shape, _lib.ptr(p), N, 0, None, 0, 9, 2, 20, 0.01, 0.0, 0, *(_lib.ptr(q) for q in out),
                                  _lib.ptr(n_iter), _lib.ptr(status), None))
    ref = tr.track_pairs(f, p, window=9, levels=2)
    assert np.array_equal(status, ref["status"]) and (status[:, [1, 4]] == 5).all() and np.array_equal(n_iter, ref["n_iter"])
    assert all(np.isnan(q[:, [1, 4]]).all() for q in out) and (n_iter[:, [1, 4]] == 0).all()
    good = [0, 2, 3]
    assert np.nanmax(np.abs(out[0][:, good] - ref["u"][:, good])) <= GATE_D


# ---- the same bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ti.CASES[2], ti.CASES[6], ti.CASES[5]], ids=ti.case_id)
def test_runs_host_twin_and_device_frames_give_the_same_bits(gpu, case):
    shape, kind, T, N, w, L = case
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    kw = ti.kwargs(case, "converge-guess")
    first = track.track_pairs(f, p, **kw)
    assert _same_tracks(track.track_pairs(f, p, **kw), first)
    assert _same_tracks(track.track_pairs(DeviceFrames.from_host(f), p, **kw), first)
    per_pair = np.broadcast_to(p, (T - 1,) + p.shape).copy()          # the same points given per pair
    assert _same_tracks(track.track_pairs(f, per_pair, **kw), first)


@pytest.mark.parametrize("device", [False, True], ids=["host", "DeviceFrames"])
def test_time_slices_with_a_halo_give_the_whole_runs_bits(gpu, device):
    shape, kind, T, N, w, L = ti.CHUNK_CASE
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    g = ti.guess_for(ti.CHUNK_CASE)
    whole = track.track_pairs(f, p, window=w, levels=L, guess=g)
    src = DeviceFrames.from_host(f) if device else f
    for cuts in ((0, 2, 4), (0, 1, 4)):                                # 2 + 2 pairs; 1 + 3: the second slice starts on an odd frame
        parts = [track.track_pairs(src[a:b + 1], p, window=w, levels=L, guess=g[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        for n in FIELDS:
            assert _same_bits(np.concatenate([getattr(q, n) for q in parts]), getattr(whole, n)), (cuts, n)


def test_workspace_batches_give_the_same_bits(gpu, monkeypatch):
    shape, kind, T, N, w, L = ti.CHUNK_CASE
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    whole = track.track_pairs(f, p, window=w, levels=L)
    whole_traj = track.trajectories(f, p, window=w, levels=L)
    per_frame = sum(h * ww for h, ww in track.level_shapes(*shape, L)[1:]) * 4
    for frames_fit in (3, 2, 0):                                       # batches of 2 pairs, of 1 pair, and a cap below the minimum of two frames
        monkeypatch.setenv("LSPIV_TRACK_WS_BYTES", str(frames_fit * per_frame))
        assert _same_tracks(track.track_pairs(f, p, window=w, levels=L), whole), frames_fit
        assert _same_tracks(track.track_pairs(DeviceFrames.from_host(f), p, window=w, levels=L), whole), frames_fit
        t = track.trajectories(f, p, window=w, levels=L)
        assert _same_bits(t.xy, whole_traj.xy) and _same_tracks(t, whole_traj), frames_fit


def test_host_upload_chunks_give_the_same_bits(gpu, monkeypatch):
    """The host twin's frames go up in chunks with one frame of halo (LSPIV_HOST_CHUNK_BYTES, default 256 MiB): pairs 2 + 2, then 1 + 1 + 1 + 1."""
    shape, kind, T, N, w, L = ti.CHUNK_CASE
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    g = ti.guess_for(ti.CHUNK_CASE)
    whole = track.track_pairs(f, p, window=w, levels=L, guess=g)
    whole_traj = track.trajectories(f, p, window=w, levels=L)
    for chunk_bytes in (3 * f[0].nbytes, 0):                           # three frames: two pairs per upload; below two frames: one pair
        monkeypatch.setenv("LSPIV_HOST_CHUNK_BYTES", str(chunk_bytes))
        assert _same_tracks(track.track_pairs(f, p, window=w, levels=L, guess=g), whole), chunk_bytes
        t = track.trajectories(f, p, window=w, levels=L)
        assert _same_bits(t.xy, whole_traj.xy) and _same_tracks(t, whole_traj), chunk_bytes


# ---- five levels (MAX_LEVELS) through the batch, chunk and chain loops: ti.FIVE_LEVEL_CASE, three frames ---------------------------------------
def test_five_levels_in_workspace_batches_give_the_same_bits(gpu, monkeypatch):
    """per_frame sums four levels: a cap of three frames (both pairs in one batch), of two frames (one pair per batch) and of 0 (below
    the minimum of two frames)."""
    shape, kind, T, N, w, L = ti.FIVE_LEVEL_CASE
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    kw = ti.kwargs(ti.FIVE_LEVEL_CASE, "converge-guess")
    whole = track.track_pairs(f, p, **kw)
    assert L == 5 == track.MAX_LEVELS and len(track.level_shapes(*shape, L)) == 5
    per_frame = sum(h * ww for h, ww in track.level_shapes(*shape, L)[1:]) * 4
    for frames_fit in (3, 2, 0):
        monkeypatch.setenv("LSPIV_TRACK_WS_BYTES", str(frames_fit * per_frame))
        assert _same_tracks(track.track_pairs(f, p, **kw), whole), frames_fit
        assert _same_tracks(track.track_pairs(DeviceFrames.from_host(f), p, **kw), whole), frames_fit


def test_five_levels_in_host_upload_chunks_give_the_same_bits(gpu, monkeypatch):
    """LSPIV_HOST_CHUNK_BYTES at three frames (both pairs in one upload) and at 0 (one pair per upload)."""
    shape, kind, T, N, w, L = ti.FIVE_LEVEL_CASE
    f, p = ti.scene(shape, T, kind), ti.points(shape, N)
    kw = ti.kwargs(ti.FIVE_LEVEL_CASE, "converge-guess")
    whole = track.track_pairs(f, p, **kw)
    for chunk_bytes in (3 * f[0].nbytes, 0):
        monkeypatch.setenv("LSPIV_HOST_CHUNK_BYTES", str(chunk_bytes))
        assert _same_tracks(track.track_pairs(f, p, **kw), whole), chunk_bytes


@pytest.mark.parametrize("device", [False, True], ids=["host", "DeviceFrames"])
def test_five_level_trajectories_are_the_references(gpu, device):
    shape, kind, T, N, w, L = ti.FIVE_LEVEL_CASE
    f, p0 = ti.scene(shape, T, kind), ti.points(shape, N)
    got = track.trajectories(DeviceFrames.from_host(f) if device else f, p0, window=w, levels=L)
    ref = ti.reference_trajectories(ti.FIVE_LEVEL_CASE)
    assert np.array_equal(got.status, ref["status"]) and np.array_equal(got.n_iter, ref["n_iter"])
    assert np.array_equal(np.isnan(got.xy), np.isnan(ref["xy"])) and np.nanmax(np.abs(got.xy - ref["xy"])) <= (T - 1) * GATE_D
    assert _same_bits(got.xy[0], p0) and (got.status[-1] < 2).any() and (got.status == tr.STATUS_BAD_POINT).any()


@pytest.mark.parametrize("device", [False, True], ids=["host", "DeviceFrames"])
def test_trajectories_are_the_loop_of_one_pair_calls(gpu, device):
    shape, kind, T, N, w, L = ti.TRAJ_CASE
    f, p0 = ti.scene(shape, T, kind), ti.points(shape, N)
    got = track.trajectories(DeviceFrames.from_host(f) if device else f, p0, window=w, levels=L)
    # the loop: pair t from row t; a lost point is not finite from then on, so it cannot be handed to track_pairs (a ValueError): it
    # keeps NaN and status 5, which is what the chain gives it
    xy = np.full((T, N, 2), np.nan)
    xy[0] = p0
    fields = {n: [] for n in FIELDS}
    for t in range(T - 1):
        alive = np.isfinite(xy[t]).all(axis=1)
        r = track.track_pairs(f[t:t + 2], xy[t][alive], window=w, levels=L)
        for n in FIELDS:
            full = np.full(N, 5 if n == "status" else 0 if n == "n_iter" else np.nan, dtype=getattr(r, n).dtype)
            full[alive] = getattr(r, n)[0]
            fields[n].append(full)
        xy[t + 1, :, 0] = xy[t, :, 0] + fields["u"][-1]
        xy[t + 1, :, 1] = xy[t, :, 1] + fields["v"][-1]
    assert _same_bits(got.xy, xy)
    for n in FIELDS:
        assert _same_bits(getattr(got, n), np.stack(fields[n])), n
    assert (got.status >= 2).any() and (got.status == 5).any() and (got.status < 2).all(axis=0).any()     # lost points included
    ref = tr.trajectories(f, p0, window=w, levels=L)
    assert np.array_equal(got.status, ref["status"]) and np.array_equal(got.n_iter, ref["n_iter"])
    assert np.array_equal(np.isnan(got.xy), np.isnan(ref["xy"])) and np.nanmax(np.abs(got.xy - ref["xy"])) <= (T - 1) * GATE_D


def test_track_grid_reproduces_the_studys_first_scene(gpu):
    """The uniform 9.3 / -6.4 px shift at density 0.02 on the 32 @ 16 grid, w = 21: the reference's shares and lost counts."""
    f = ti.study_scene("shift", 0.02)
    pts, (rows, cols) = tr.grid_points(*ti.STUDY_SHAPE, 32, 16)
    truth = ti.study_truth("shift", pts)
    for levels in (1, 3, 4):
        g = track.track_grid(f, 32, 16, window=21, levels=levels)
        assert g.u.shape == (1, rows, cols) and g.u32.dtype == np.float32 and _same_bits(g.u32, g.u.astype(np.float32)) and _same_bits(g.v32, g.v.astype(np.float32))
        ref = tr.track_pairs(f, pts, window=21, levels=levels)
        assert ref["margins"].smallest() > 1e-8
        got = {n: getattr(g, n).reshape(1, -1) for n in FIELDS}
        assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_iter"], ref["n_iter"])
        assert ti.study_figures(got, truth)[::2] == ti.study_figures(ref, truth)[::2]        # the share within 0.5 px and the lost count
        assert np.nanmax(np.abs(got["u"] - ref["u"])) <= GATE_D and np.nanmax(np.abs(got["v"] - ref["v"])) <= GATE_D
    xx, yy = np.meshgrid(g.x, g.y)
    assert np.array_equal(np.stack([xx.ravel(), yy.ravel()], axis=1), pts)
