"""Float64 reference of the sliding ensemble, composed of the oracle as it stands: output j is the
oracle's own ensemble over the frames of its M pairs, in ONE chunk -- the oracle's ``n_frames`` is then 1, hence ``count_min * M``.
Like the rest of the PIV path it is this project's reading: unpinned against a real ffpiv.

Also the inputs of tests/test_gpu_sliding.py (``CASES``, ``case_stack``, ``blanked_stack``, ``speckle_stack``, ``signal_stack``) and
their references, computed once per process (``case_ref``, ...) and shared by the CPU checks of the inputs (tests/test_sliding_host.py) and the GPU tests."""
import functools

import numpy as np

from oracle import piv_oracle as po
from pyorc_amd.synth import particle_stack

KW = dict(corr_min=0.1, s2n_min=1.5, count_min=0.2)


def sliding_piv(frames, dt, window, overlap, M, s, res=1.0, time=None, corr_min=0.2, s2n_min=3.0, count_min=0.2, signal_threshold=None):
    """dict(v_x, v_y, corr, s2n (n_out, n_rows, n_cols), planes (n_out, n_win, wy, wx), count, tie (n_out, n_rows, n_cols), time, dt)."""
    frames = np.asarray(frames)
    dt = np.asarray(dt, dtype=np.float64)
    P = frames.shape[0] - 1
    n_out = P // s - M // s + 1
    assert n_out >= 1
    t2 = (np.arange(P + 1, dtype=np.float64) if time is None else np.asarray(time, dtype=np.float64))[1:]
    out = {k: [] for k in ("v_x", "v_y", "corr", "s2n", "planes")}
    for j in range(n_out):
        r = po.get_ffpiv(frames[j * s:j * s + M + 1], dt[j * s:j * s + M], window, overlap, res, res, ensemble_corr=True, chunksize=None,
                         corr_min=corr_min, s2n_min=s2n_min, count_min=count_min * M, signal_threshold=signal_threshold)
        for k in ("v_x", "v_y", "corr", "s2n"):
            out[k].append(np.asarray(r[k])[0])
        out["planes"].append(np.asarray(r["corr_mean"])[0])
    out = {k: np.stack(v) for k, v in out.items()}
    shape = out["v_x"].shape
    # pairs kept per (output, window): the masks of the ensemble branch on the oracle's own per-pair corr_max / s2n
    pp = po.get_ffpiv(frames, dt, window, overlap, res, res, signal_threshold=signal_threshold)
    cm, sn = np.asarray(pp["corr"], dtype=np.float64), np.asarray(pp["s2n"], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        kept = (cm >= corr_min) & (sn >= s2n_min) & np.isfinite(cm) & (cm > 1e-6)
    out["count"] = np.stack([kept[j * s:j * s + M].sum(axis=0) for j in range(n_out)]).astype(np.float64)
    top = np.sort(out["planes"].reshape(out["planes"].shape[:2] + (-1,)), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        out["tie"] = (((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (top[..., 1] > 0)).reshape(shape)
    out["time"] = np.array([t2[j * s:j * s + M].mean() for j in range(n_out)])
    out["dt"] = np.array([dt[j * s:j * s + M].mean() for j in range(n_out)])
    return out


# (id, window, overlap, (H, W), frames): every kernel family of the ensemble mode.  The walking kernels 32 / 64 / 16, a prime-factor
# size, and the families that take one launch per block: embedded 15, direct 12 x 20, the LDS-resident DFT 72 (needs larger frames).
CASES = {
    "32-16": ((32, 32), (16, 16), (70, 90), 13),
    "64-48": ((64, 64), (48, 48), (96, 130), 13),
    "16-8": ((16, 16), (8, 8), (70, 90), 13),
    "24-12": ((24, 24), (12, 12), (70, 90), 13),
    "15-7": ((15, 15), (7, 7), (70, 90), 13),
    "12x20": ((12, 20), (6, 10), (70, 90), 13),
    "72-36": ((72, 72), (36, 36), (150, 190), 13),
}
SEEDS = {"32-16": 11, "64-48": 12, "16-8": 13, "24-12": 14, "15-7": 15, "12x20": 16, "72-36": 17}
DTYPES = (np.uint8, np.float32)
# (case, M, s) of the parity test
PARITY = [(c, 4, 2) for c in CASES] + [("32-16", 6, 1), ("32-16", 6, 6)]


def as_samples(a, dtype):
    """uint8 as drawn; float32 signed, through an affine map (the same normalised windows)."""
    return a if dtype == np.uint8 else a.astype(dtype) * dtype(0.37) - dtype(11.0)


@functools.lru_cache(maxsize=None)
def case_stack(case, dtype=np.uint8):
    _, _, (H, W), T = CASES[case]
    return as_samples(particle_stack(T, H, W, seed=SEEDS[case], density=0.05), dtype)


@functools.lru_cache(maxsize=None)
def case_ref(case, dtype, M, s):
    window, overlap, _, T = CASES[case]
    return sliding_piv(case_stack(case, dtype), np.ones(T - 1), window, overlap, M, s, **KW)


@functools.lru_cache(maxsize=None)
def blanked_stack():
    """The 32 / 16 stack with the particles of the left half blanked in frames 5 .. 9: the windows there lose the pairs 4 .. 9."""
    a = case_stack("32-16").copy()
    a[5:10, :, :45] = 0
    return a


COUNT_KW = dict(corr_min=0.1, s2n_min=1.5, count_min=0.5)


@functools.lru_cache(maxsize=None)
def blanked_ref():
    return sliding_piv(blanked_stack(), np.ones(12), (32, 32), (16, 16), 4, 2, **COUNT_KW)


# ---- the float64 rescue per output: a stack that provably has ill-conditioned fits ------------------------------------------
RESCUE = ((32, 32), (16, 16), 4, 2)      # window, overlap, M, s
RESCUE_CHUNKS = [(0, 5), (4, 9)]         # two accumulate calls of 4 pairs: output 1 = pairs [2, 6) straddles them, the second starts at pair 4


@functools.lru_cache(maxsize=None)
def speckle_stack(T=9, H=200, W=264, seed=11, stepped=False):
    """The recipe of tests/test_gpu_parity.py (``_speckle_and_particles``).  Left part: one single-pixel speckle per 16 x 16 cell
    drifting one pixel per frame -- every correlation peak sits on exactly-zero neighbours, the worst case of the float32 fit, so
    windows are flagged; right part: an ordinary sparse particle image.
    ``stepped``: the speckles jump one pixel further at every 8th frame and, after frame 20, at every 3rd: a pair across a jump moves
    2 px (3 px at frame 32), so a mean plane has its peak at 1 px, a smaller one at 2 px and exactly zero on the other side -- still the
    worst case of the float32 fit, but the fit now depends on WHICH pairs are in the sum."""
    rng = np.random.default_rng(seed)
    fr = particle_stack(T, H, W, seed=seed, density=0.012)
    half = (W // 32) * 16
    fr[:, :, :half] = 0
    ys, xs = np.meshgrid(np.arange(8, H, 16), np.arange(8, half - 8, 16), indexing="ij")
    amp = rng.integers(100, 255, ys.shape)
    for t in range(T):
        fr[t, ys, xs + t + (t // 8 + max(0, t - 20) // 3 if stepped else 0)] = amp
    return fr


@functools.lru_cache(maxsize=None)
def speckle_ref():
    window, overlap, M, s = RESCUE
    a = speckle_stack()
    return sliding_piv(a, np.ones(len(a) - 1), window, overlap, M, s, **KW)


# ---- signal thresholds, both signal modes -----------------------------------------------------------------------------------
SIGNAL_THR = 0.2


@functools.lru_cache(maxsize=None)
def signal_stack():
    """The 32 / 16 stack with an empty corner in every frame (that window position fails the threshold in both signal modes) and
    frame 6 empty from column 38 on (pair mode drops the pairs 5 and 6 of the windows there; position mode keeps them)."""
    a = case_stack("32-16").copy()
    a[:, :34, :34] = 0
    a[6, :, 38:] = 0
    return a


@functools.lru_cache(maxsize=None)
def signal_ref(mode):
    """Under ``signal_mode`` = mode.  Mode 1 scores a window position over the frames of ONE call: the reference's call holds an
    output's frames, the device's the whole stack -- tests/test_sliding_host.py checks that both keep the same positions here."""
    with po.semantics(signal_mode=mode):
        return sliding_piv(signal_stack(), np.ones(12), (32, 32), (16, 16), 4, 2, signal_threshold=SIGNAL_THR, **KW)


# ---- more than one tile of outputs, pair-block and kept chunk: the inputs of tests/test_gpu_batch_loops.py ----------------------------------
# (case: frames, M, s, the two accumulate calls).  "long": 40 pairs, 10 blocks, 6 outputs; the rescue sums in blocks of 16 pairs per kept
# chunk: outputs 0 .. 3 straddle pair 16, output 4 = pairs [16, 36) straddles pair 32; in two calls of 20 pairs each chunk holds the
# ragged blocks 16 + 4.  "many": 35 pairs, 17 blocks, 16 outputs
# "stepped": "long" on the stepped stack -- the flagged windows of "long" and "many" have the same fit whichever pairs are summed (every
# pair moves 1 px), those of "stepped" do not: an output that sums another output's pairs, or drops a pair-block, moves
LOOP_CASES = {"long": (41, 20, 4, [(0, 21), (20, 41)], False), "many": (36, 4, 2, [(0, 17), (16, 36)], False),
              "stepped": (41, 20, 4, [(0, 21), (20, 41)], True)}
LOOP_WINDOW = ((32, 32), (16, 16))


@functools.lru_cache(maxsize=None)
def loop_ref(case):
    T, M, s, _, stepped = LOOP_CASES[case]
    return sliding_piv(speckle_stack(T=T, stepped=stepped), np.ones(T - 1), *LOOP_WINDOW, M, s, **KW)
