"""The geometry sweep of the mode PIV kernels (shifted pass, window deformation, SPOF, image mask, second peak and the shifted and SPOF
ensemble passes; INTEGRATION.md sections 2d - 2i): frames, overlaps and grids the parity inputs of those modes (``ensemble_multipass_ref.
PASS_CASES``: strides of 8, 16 and 32 px, oy == ox, three to seven windows per side) do not reach -- one window, one row, one column,
stride 1, odd strides, oy != ox, an unread margin, and nine blocks at every size -- with the stacks, offsets, nodes, masks and float64
references tests/test_mode_geometry_host.py (CPU) and tests/test_gpu_mode_geometry.py share, computed once per process and never changed."""
import functools
from collections import namedtuple

import numpy as np

from pyorc_amd import synth
from tests import deform_ref, masked_ref, peak2_ref, spof_ref
from tests import ensemble_multipass_ref as emp
from tests import multipass_ref as mp

SIZES = (16, 32, 64)
DTYPES = (np.uint8, np.float32, np.float64)
DTYPE_IDS = ("u8", "f32", "f64")
SHIFT = emp.PASS_SHIFT                      # (dx, dy) = (3, -2): the stacks' uniform displacement
DENSITY = 0.05
SIGNAL_THR = deform_ref.SIGNAL_THR          # 0.3
WAVES_PER_BLOCK = 4                         # the skeleton's: a block holds 4 waves of 64 / n windows each
# "blocks": 3 * rows * cols jobs that need nine blocks, the last one partly filled -- 132, 66 and 33 jobs at 16, 8 and 4 per block
BLOCK_DIMS = {16: (43, 97), 32: (51, 193), 64: (67, 385)}
WILD = ((-300, 300), (32767, -32768))       # offsets {dy, dx} far outside any frame: the kernel clamps them

Geometry = namedtuple("Geometry", "name n dim overlap T")      # overlap: (oy, ox)


def sweep(n):
    """The eight geometries of window size n."""
    h = n // 2
    return (Geometry("one-window", n, (n, n), (0, 0), 3),                              # 1 x 1 grid, every block mostly tail
            Geometry("row-stride-1", n, (n, n + 7), (n - 1, n - 1), 3),                # origins at every byte alignment, one row
            Geometry("col-stride-1", n, (n + 5, n), (n - 1, n - 1), 2),                # one column, a single pair
            Geometry("odd-stride", n, (2 * n + 5, 3 * n + 3), (h + 3, h + 3), 4),      # odd stride, odd row pitch
            Geometry("ragged-0", n, (2 * n + h + 1, 4 * n - 1), (0, 0), 3),            # unread margin on both axes
            Geometry("blocks", n, BLOCK_DIMS[n], (h, h), 4),                           # 9 blocks, last one partial
            Geometry("asym", n, (2 * n + 5, 3 * n + 3), (h + 3, 1), 3),                # oy != ox
            Geometry("asym-T", n, (3 * n + 3, 2 * n + 5), (0, n - 3), 3))              # its transpose


NAMES = tuple(g.name for g in sweep(16))
GEOMETRIES = {(g.name, n): g for n in SIZES for g in sweep(n)}
KEYS = tuple(GEOMETRIES)
IDS = tuple(f"{n}-{name}" for name, n in KEYS)
# the deformation pass takes one overlap for both axes (its node grid has one stride): the two asymmetric geometries are refused there
SYM_KEYS = tuple(k for k in KEYS if GEOMETRIES[k].overlap[0] == GEOMETRIES[k].overlap[1])
SYM_IDS = tuple(f"{n}-{name}" for name, n in SYM_KEYS)
NAN_NAMES = ("row-stride-1", "odd-stride")   # the overlapping geometries of the NaN-sample test

# seeds: 1000 + n + H + W unless a reference of that stack holds a tie or a fragile window the gates would have to set aside on a small
# grid (tests/test_mode_geometry_host.py states the rule and checks it; the replacements were searched on the CPU, upwards from the formula's)
SEEDS = {("odd-stride", 16): 1109,       # the formula's 1106: 1 fragile SPOF window in 120, 0.8 % against a cap of 1 %
         ("asym-T", 16): 1105,           # 1104: 1 fragile second peak in 48
         ("one-window", 32): 1103,       # 1096: an exact tie in one of the two deformed planes
         ("row-stride-1", 32): 1104,     # 1103: 1 fragile second peak in 16 on the signal stack
         ("blocks", 32): 1280,           # 1276: 1 fragile second peak in 66
         ("asym-T", 32): 1207,           # 1200: 2 fragile second peaks in 78
         ("odd-stride", 64): 1395,       # 1392: 2 fragile second peaks in 45
         ("asym", 64): 1394}             # 1392: 3 fragile second peaks in 18


def seed(key):
    g = GEOMETRIES[key]
    return SEEDS.get(key, 1000 + g.n + g.dim[0] + g.dim[1])


def grid(key):
    g = GEOMETRIES[key]
    y0, x0 = mp.grid_origins(g.dim, g.n, g.overlap)
    return len(y0), len(x0)


def jobs_per_block(n):
    return WAVES_PER_BLOCK * 64 // n


def blocks(key):
    """(jobs, blocks, jobs in the last block) of a per-pair launch: one window per job."""
    g = GEOMETRIES[key]
    rows, cols = grid(key)
    jobs, per = (g.T - 1) * rows * cols, jobs_per_block(g.n)
    nb = -(-jobs // per)
    return jobs, nb, jobs - (nb - 1) * per


@functools.lru_cache(maxsize=None)
def stack_u8(key, seed_=None):
    g = GEOMETRIES[key]
    return synth.particle_stack(g.T, g.dim[0], g.dim[1], seed=seed(key) if seed_ is None else seed_, density=DENSITY,
                                uniform_shift=(float(SHIFT[0]), float(SHIFT[1])))


@functools.lru_cache(maxsize=None)
def stack(key, dtype=np.uint8, seed_=None):
    return emp.as_samples(stack_u8(key, seed_), dtype)


@functools.lru_cache(maxsize=None)
def signal_stack(key, seed_=None):
    """The recipe of deform_ref.signal_stack: samples below 40 set to zero, the upper left quarter of every frame empty; uint8."""
    a = stack_u8(key, seed_).copy()
    a[a < 40] = 0
    a[:, :a.shape[1] // 2, :a.shape[2] // 2] = 0
    return a


@functools.lru_cache(maxsize=None)
def offsets(key):
    """int16 (P, rows, cols, 2) {dy, dx}: the uniform shift +-3 per window and pair, and two entries far outside the frame (the first
    and the last one)."""
    g = GEOMETRIES[key]
    rows, cols = grid(key)
    rng = np.random.default_rng(100 + g.n + rows * cols)
    sh = np.empty((g.T - 1, rows, cols, 2), dtype=np.int16)
    sh[..., 0] = SHIFT[1] + rng.integers(-3, 4, sh.shape[:3])
    sh[..., 1] = SHIFT[0] + rng.integers(-3, 4, sh.shape[:3])
    sh[0, 0, 0] = WILD[0]
    sh[-1, -1, -1] = WILD[1]
    return sh


@functools.lru_cache(maxsize=None)
def nodes(key):
    """int32 (P, rows, cols, 2) {v, u} in 1 / 128 px: the uniform shift +-1.5 px per window and pair, and two entries of tens of pixels
    (the first and the last one) that push samples across the frame edge."""
    g = GEOMETRIES[key]
    rows, cols = grid(key)
    rng = np.random.default_rng(300 + g.n + rows * cols)
    out = np.empty((g.T - 1, rows, cols, 2), dtype=np.int32)
    out[..., 0] = np.rint(128 * (SHIFT[1] + rng.uniform(-1.5, 1.5, out.shape[:3])))
    out[..., 1] = np.rint(128 * (SHIFT[0] + rng.uniform(-1.5, 1.5, out.shape[:3])))
    out[0, 0, 0] = (-40 * 128, -25 * 128)
    out[-1, -1, -1] = (33 * 128 + 7, 60 * 128 + 1)
    return out


@functools.lru_cache(maxsize=None)
def mask(key):
    return masked_ref.parity_mask(*GEOMETRIES[key].dim)


def radii(n):
    return (1, n // 4)


# ---- the float64 references -------------------------------------------------------------------------------------------------------------
def _f64(a):
    return a if a.dtype == np.uint8 else a.astype(np.float64)


MODES = ("shifted", "deformed", "spof", "masked", "peak2-1", "peak2-q")     # peak2 at radius 1 and n / 4
ENSEMBLES = ("shifted-ensemble", "spof-ensemble")
SPOF_ENS_KW = dict(corr_min=0.0, s2n_min=0.5, count_min=0.2)                # like emp.OPEN_KW: masks that keep every pair


def compute(mode, key, a, signal_threshold=None):
    """The reference of ``mode`` at the geometry ``key`` on the stack ``a`` (in its own sample type)."""
    g = GEOMETRIES[key]
    if mode == "shifted":
        return mp.shifted_piv(_f64(a), g.n, g.overlap, offsets(key), signal_threshold)
    if mode == "unshifted":
        return mp.shifted_piv(_f64(a), g.n, g.overlap, None, signal_threshold)
    if mode == "deformed":
        return deform_ref.deformed_piv(a, g.n, g.overlap, nodes(key), signal_threshold)
    if mode == "undeformed":
        return deform_ref.deformed_piv(a, g.n, g.overlap, None, signal_threshold)
    if mode == "spof":
        return spof_ref.piv(a, g.n, g.overlap, signal_threshold)
    if mode == "masked":
        return masked_ref.piv(a, g.n, g.overlap, mask(key), signal_threshold=signal_threshold)
    if mode in ("peak2-1", "peak2-q"):
        return peak2_ref.piv(a, g.n, g.overlap, radii(g.n)[mode == "peak2-q"], signal_threshold)
    if mode == "shifted-ensemble":
        return emp.ensemble_pass(_f64(a), g.n, g.overlap, offsets(key)[0], n_frames=1, signal_threshold=signal_threshold, **emp.OPEN_KW)
    if mode == "spof-ensemble":
        return spof_ref.ensemble(a, g.n, g.overlap, n_frames=1, signal_threshold=signal_threshold, **SPOF_ENS_KW)
    raise ValueError(mode)


@functools.lru_cache(maxsize=None)
def ref(mode, key, dtype=np.uint8):
    return compute(mode, key, stack(key, dtype))


@functools.lru_cache(maxsize=None)
def signal_ref(mode, key):
    return compute(mode, key, signal_stack(key), SIGNAL_THR)


def set_aside(mode, r):
    """(windows the mode's gate may set aside, windows it is held on) of a reference: exact ties for the shifted and deformed passes and the
    shifted ensemble, ties and fragile windows for the masked pass, fragile windows for SPOF and its ensemble, ``fragile2`` among the kept
    windows for the second peak."""
    kept = np.isfinite(r["corr"])
    if mode in ("shifted", "unshifted", "deformed", "undeformed", "shifted-ensemble"):
        bad = r["tie"]
    elif mode == "masked":
        bad = r["tie"] | r["fragile"]
    elif mode in ("spof", "spof-ensemble"):
        bad = r["fragile"]
    else:
        bad = r["fragile2"]
    if mode.startswith("peak2"):           # (its gate counts among the windows that are not skipped)
        return int((bad & kept).sum()), int(kept.sum())
    return int(bad.sum()), int(bad.size)


def modes_of(key):
    return tuple(m for m in MODES + ENSEMBLES if m != "deformed" or key in SYM_KEYS)


# ---- one NaN sample ---------------------------------------------------------------------------------------------------------------------
def windows_holding(key, y, x):
    """(rows, cols) bool: the windows whose rectangle contains the sample (y, x), from the origins alone."""
    g = GEOMETRIES[key]
    y0, x0 = mp.grid_origins(g.dim, g.n, g.overlap)
    return ((y0 <= y) & (y < y0 + g.n))[:, None] & ((x0 <= x) & (x < x0 + g.n))[None, :]


@functools.lru_cache(maxsize=None)
def nan_sample(key):
    """(y, x): the first valid sample of the mask, in row-major order from the frame's middle row downwards, that several windows read but
    not all of them."""
    g = GEOMETRIES[key]
    m = mask(key)
    rows, cols = grid(key)
    for y in list(range(g.dim[0] // 2, g.dim[0])) + list(range(g.dim[0] // 2)):
        for x in range(g.dim[1]):
            if m[y, x] and 2 <= windows_holding(key, y, x).sum() < rows * cols:
                return y, x
    raise ValueError(f"{key}: no such sample")
