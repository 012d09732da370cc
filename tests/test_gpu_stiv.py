"""GPU tests of space-time image velocimetry against tests/stiv_ref.py: the gather bit for bit (every kind
of line, both dtypes, chunks through t_offset, host stacks and DeviceFrames), the orientation within the reference's gates on the inputs
that tests/test_stiv_host.py qualified, NaN where the reference has NaN, the same bits from run to run and from the host twin, and the
whole mode on the river scene."""
import numpy as np
import pytest

from pyorc_amd import DeviceFrames, stiv
from tests import stiv_ref as sr

pytestmark = pytest.mark.gpu

SHAPES = ((48, 64), (33, 47))
SAMPLES = (3, 37, 64, 65, 130)       # below, at and above a wave, no multiple of it, more than two waves
FRAME_COUNTS = (3, 7, 33)            # below, above and far above the kernel's four frames per trip, none a multiple of four


def _lines(H, W):
    """Five lines: horizontal at fractional offsets; vertical, ending exactly on the last row; the diagonal, ending exactly on the last
    row and column; an oblique one walked backwards from the last column; a zero-length line on the frame's last pixel."""
    return np.array([[0.3, 5.25, W - 1.7, 5.25],
                     [7.5, 0.0, 7.5, H - 1.0],
                     [0.0, 0.0, W - 1.0, H - 1.0],
                     [W - 1.0, H - 1.5, 1.25, 2.0],
                     [W - 1.0, H - 1.0, W - 1.0, H - 1.0]])


def _frames(dtype, T, shape, special=False):
    rng = np.random.default_rng(T * 1000 + shape[0])
    f = rng.integers(0, 256, size=(T,) + shape)
    if dtype == np.uint8:
        return f.astype(np.uint8)
    f = (f + rng.random(f.shape) - 100.0).astype(np.float32)
    if special:
        kind = rng.random(f.shape)
        f[kind < 0.03] = np.nan
        f[(kind >= 0.03) & (kind < 0.10)] = 0.0
        f[(kind >= 0.10) & (kind < 0.17)] = -0.0
        f[:, -1, -1] = -0.0          # the zero-length line sits here: -0 blended with itself
    return f


def _same_bits(got, want):
    """Equal bit for bit (the sign of a zero included); a NaN must be a NaN (its payload is the hardware's own)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    kind = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(kind)[~nan], want.view(kind)[~nan])


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", ["uint8", "float32", "float32-nan-zeros"])
def test_gather_is_the_references_bits(gpu, case, shape):
    dtype = np.uint8 if case == "uint8" else np.float32
    lines = _lines(*shape)
    for T in FRAME_COUNTS:
        f = _frames(dtype, T, shape, special=case.endswith("zeros"))
        for L in SAMPLES:
            for ln in (lines, lines[2:3]):          # S = 5 and S = 1
                want = sr.space_time_images(f, sr.line_points(ln, L))
                got = stiv.space_time_images(f, ln, L)
                assert _same_bits(got, want), (T, L, len(ln))
    if case.endswith("zeros"):          # the case is what it says (a blend of zeros of either sign is +0 here and there alike)
        assert np.isnan(f).any() and np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all() and np.isnan(want).any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_chunks_through_t_offset_fill_the_same_image(gpu, dtype):
    shape, L = SHAPES[1], 65
    lines = _lines(*shape)
    for T in (7, 33):
        f = _frames(dtype, T, shape)
        want = sr.space_time_images(f, sr.line_points(lines, L))
        d = DeviceFrames.from_host(f)
        whole = stiv.space_time_images(d, lines, L)
        assert isinstance(whole, DeviceFrames) and whole.shape == want.shape and _same_bits(whole.to_host(), want)
        for step in (1, 2, T):
            out = np.full(want.shape, -7.0, dtype=np.float32)
            d_out = DeviceFrames.from_host(out)
            for a in range(0, T, step):
                assert stiv.space_time_images(f[a:a + step], lines, L, out=out, t_offset=a) is out
                assert stiv.space_time_images(d[a:a + step], lines, L, out=d_out, t_offset=a) is d_out
            assert _same_bits(out, want) and _same_bits(d_out.to_host(), want), (T, step)
    # rows outside [t_offset, t_offset + T) are left alone
    out = np.full((5, T + 3, L), -7.0, dtype=np.float32)
    d_out = DeviceFrames.from_host(out)
    stiv.space_time_images(f, lines, L, out=out, t_offset=2)
    stiv.space_time_images(d, lines, L, out=d_out, t_offset=2)
    for got in (out, d_out.to_host()):
        assert _same_bits(got[:, 2:T + 2], want) and (got[:, :2] == -7.0).all() and (got[:, T + 2:] == -7.0).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_host_upload_chunks_give_the_references_bits(gpu, monkeypatch, dtype):
    """The host twin's frames go up in chunks (LSPIV_HOST_CHUNK_BYTES, default 256 MiB): 2 + 2 + 2 + 1 frames, then one frame at a time."""
    shape, T, L = SHAPES[1], 7, 65
    lines = _lines(*shape)
    f = _frames(dtype, T, shape)
    want = sr.space_time_images(f, sr.line_points(lines, L))
    for chunk_bytes in (2 * f[0].nbytes, 1):                           # two frames; below one frame: chunks of one frame
        monkeypatch.setenv("LSPIV_HOST_CHUNK_BYTES", str(chunk_bytes))
        assert _same_bits(stiv.space_time_images(f, lines, L), want), chunk_bytes
        out = np.full((len(lines), T + 3, L), -7.0, dtype=np.float32)
        assert stiv.space_time_images(f, lines, L, out=out, t_offset=2) is out
        assert _same_bits(out[:, 2:T + 2], want) and (out[:, :2] == -7.0).all() and (out[:, T + 2:] == -7.0).all(), chunk_bytes


# ---- orientation ------------------------------------------------------------------------------------------------------------------------
def _within_gates(got, ref):
    """NaN exactly where the reference has it, everything else within the gates; returns the worst tensor error over the trace."""
    tensor, slope, coh = ref
    assert got.tensor.shape == tensor.shape and got.slope.shape == slope.shape and got.coherency.shape == coh.shape
    assert np.array_equal(np.isnan(got.tensor), np.isnan(tensor))
    assert np.array_equal(np.isnan(got.slope), np.isnan(slope)) and np.array_equal(np.isnan(got.coherency), np.isnan(coh))
    trace = tensor[..., 0] + tensor[..., 1]
    ok = np.isfinite(trace) & (trace > 0)
    assert np.array_equal(got.tensor[trace == 0], tensor[trace == 0])          # a constant window: zeros
    ratio = np.abs(got.tensor[ok] - tensor[ok]) / trace[ok][:, None]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= sr.GATE_TENSOR
    fin = np.isfinite(slope)
    assert (np.abs(got.slope[fin] - slope[fin]) <= sr.GATE_SLOPE * (1.0 + slope[fin] ** 2)).all()
    assert (np.abs(got.coherency[fin] - coh[fin]) <= sr.GATE_COHERENCY).all()
    return worst


@pytest.mark.parametrize("case", sr.PARITY_CASES, ids=lambda c: "S{}-T{}-L{}-Tw{}-st{}-k{}-{}".format(*c[:6], "detrend" if c[8] else "plain"))
def test_orientation_agrees_with_the_reference(gpu, case):
    S, T, L, Tw, stride, k, omega, m0, detrend = case
    sti = sr.moving_texture(S, T, L, omega, m0)
    ref = sr.orientation(sti, Tw, stride, k, detrend)
    assert np.isfinite(ref[1]).all()
    d_sti = DeviceFrames.from_host(sti)
    dev = stiv.orientation(d_sti, Tw, stride, k, detrend)
    worst = _within_gates(dev, ref)
    print(f"worst |J - J_ref| / (Jxx + Jtt) = {worst:.2e}")
    again, host = stiv.orientation(d_sti, Tw, stride, k, detrend), stiv.orientation(sti, Tw, stride, k, detrend)
    for a, b, c in zip(dev, again, host):          # two runs, and the host twin: the same bits
        assert _same_bits(a, b) and _same_bits(a, c)


def test_orientation_defaults_are_one_window_smooth_1_detrended(gpu):
    sti = sr.moving_texture(5, 33, 65, 1.0, 0.5)
    got = stiv.orientation(sti)
    assert got.slope.shape == (5, 1)
    _within_gates(got, sr.orientation(sti, 33, 33, 1, True))


def test_nan_is_where_the_reference_has_it(gpu):
    const = np.full((2, 9, 12), 100.0, dtype=np.float32)          # a constant stack: 0 / 0
    for detrend in (True, False):
        got = stiv.orientation(const, smooth=1, detrend=detrend)
        _within_gates(got, sr.orientation(const, smooth=1, detrend=detrend))
        assert np.isnan(got.slope).all() and np.isnan(got.coherency).all() and not got.tensor.any()
    sti = sr.moving_texture(5, 33, 65, 1.0, 0.5).copy()
    sti[2, 15, 30] = np.nan                                       # inside window 1 of line 2 only
    for detrend in (True, False):
        ref = sr.orientation(sti, 11, 11, 1, detrend)
        want = np.zeros((5, 3), dtype=bool)
        want[2, 1] = True
        assert np.array_equal(np.isnan(ref[1]), want)
        got = stiv.orientation(sti, 11, 11, 1, detrend)
        _within_gates(got, ref)
        assert np.array_equal(np.isnan(got.slope), want) and np.array_equal(np.isnan(got.coherency), want)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_stiv_on_the_river_scene(gpu):
    """The first scene of tests/test_stiv_host.py: the GPU equals the reference within the gates, so the reference's accuracy carries."""
    frames = sr.river_scene(1, 6.0)
    lines, truth = sr.scene_lines()
    L, res, dt = sr.SCENE_SAMPLES, 0.01, 0.04
    v, slope, coh, tensor, ds = sr.stiv(frames, lines, L, resolution=res, dt=dt)
    for stack in (frames, DeviceFrames.from_host(frames)):
        got = stiv.stiv(stack, lines, L, resolution=res, dt=dt)
        _within_gates(stiv.Orientation(got.tensor, got.slope, got.coherency), (tensor, slope, coh))
        assert np.array_equal(got.ds, ds)
        assert np.array_equal(got.v, sr.velocity(got.slope, got.ds, res, dt))       # one float64 chain: (slope ds) resolution / dt
        np.testing.assert_allclose(got.v, v, rtol=0, atol=sr.GATE_SLOPE * (1.0 + np.abs(slope).max() ** 2) * res / dt)
        assert np.median(np.abs(got.slope[:, 0] - truth)) < 0.1
    # half the samples on the same lines: ds = 2, half the slope, the same velocity chain
    coarse = stiv.stiv(frames, lines, 65, smooth=1, resolution=res, dt=dt)
    assert np.array_equal(coarse.ds, np.full(14, 2.0)) and np.array_equal(coarse.v, sr.velocity(coarse.slope, coarse.ds, res, dt))
    ref = sr.stiv(frames, lines, 65)
    _within_gates(stiv.Orientation(coarse.tensor, coarse.slope, coarse.coherency), (ref[3], ref[1], ref[2]))
