"""Mirror of ``ffpiv.window`` for the call sites on pyorc's PIV path.

Reference call sites: pyorc/api/frames.py:85-90 (``get_rect_coordinates``), :167
(``round_to_even``); pyorc/velocimetry/ffpiv.py:120-126 (``required_memory``), :129
(``available_memory``).  The grid functions call the C ABI (host-only code in
liblspiv_hip.so, no GPU needed); the memory functions answer for HBM instead of host RAM,
because that is what bounds a chunk on the ``hip`` engine.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib


def round_to_even(input_tuple: Sequence[float]) -> Tuple[int, ...]:
    """Round window sizes to even integers (pyorc/api/frames.py:167).  The direction for odd sizes is the
    library option ``round_odd``: 0 round-half-even of x / 2 (25 -> 24, 27 -> 28; default), 1 up, 2 down."""
    mode = _lib.get_option("round_odd")
    if mode == 1:
        return tuple(int(np.ceil(float(x) / 2.0) * 2) for x in input_tuple)
    if mode == 2:
        return tuple(int(np.floor(float(x) / 2.0) * 2) for x in input_tuple)
    return tuple(int(np.round(float(x) / 2.0) * 2) for x in input_tuple)


SEARCH_AREAS = (16, 32, 64)


class SearchWindow(tuple):
    """A window searched inside a larger search area, as ONE window argument of the layers below ``get_ffpiv`` / ``piv_pairs``: the tuple
    itself is the SEARCH AREA ``(say, sax)`` -- which lays out the grid, the correlation planes and the memory plan, so every
    function that takes a window size answers for the search area --, ``.window`` the ``(wy, wx)`` cut from frame t."""

    def __new__(cls, search_area, window):
        self = super().__new__(cls, (int(search_area[0]), int(search_area[1])))
        self.window = (int(window[0]), int(window[1]))
        return self


def search_spec(window_size, search_area_size=None):
    """``window_size`` as the layers below take it: the plain tuple when there is no search area of its own (None, or equal to the
    window: today's path), else a validated :class:`SearchWindow`.  Host-only.  Supported: a square search area of 16, 32 or 64 px
    with a square even window, 4 <= window <= search area - 2; not with the option ``norm_clip`` = 0."""
    if isinstance(window_size, SearchWindow):
        return window_size
    ws = (int(window_size[0]), int(window_size[1]))
    if search_area_size is None or (int(search_area_size[0]), int(search_area_size[1])) == ws:
        return ws
    sa = (int(search_area_size[0]), int(search_area_size[1]))
    if not _lib.load().lspiv_search_supported(sa[0], sa[1], ws[0], ws[1]):
        raise ValueError(f"search_area_size {sa} with window_size {ws} is not supported: the search area must be square and one of "
                         f"{SEARCH_AREAS}, the window square and even with 4 <= window <= search area - 2 (or search_area_size == "
                         "window_size)")
    if _lib.get_option("norm_clip") == 0:
        raise ValueError("option norm_clip = 0 is served by the block-per-window kernels only, not with a search_area_size "
                         "larger than the window")
    return SearchWindow(sa, ws)


def get_axis_shape(dim_size: int, window_size: int, overlap: int) -> int:
    nr, nc = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_grid_shape(dim_size, dim_size, window_size, window_size, overlap, overlap,
                                            C.byref(nr), C.byref(nc)))
    return nr.value


def get_array_shape(dim_size, window_size, overlap) -> Tuple[int, int]:
    nr, nc = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_grid_shape(dim_size[0], dim_size[1], window_size[0], window_size[1],
                                            overlap[0], overlap[1], C.byref(nr), C.byref(nc)))
    return nr.value, nc.value


def get_rect_coordinates(dim_size, window_size, overlap, search_area_size=None, center_on_field=False):
    """Window-centre pixel indices ``(x_cols, y_rows)``, int64 (usable for fancy indexing)."""
    if center_on_field:
        raise NotImplementedError("pyorc never centres the grid on the field")
    sa = window_size if search_area_size is None else search_area_size
    n_rows, n_cols = get_array_shape(dim_size, sa, overlap)
    rows = np.empty(max(n_rows, 0), dtype=np.int64)
    cols = np.empty(max(n_cols, 0), dtype=np.int64)
    _lib.check(_lib.load().lspiv_grid_coords(dim_size[0], dim_size[1], sa[0], sa[1], overlap[0], overlap[1],
                                             rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                             cols.ctypes.data_as(C.POINTER(C.c_int64))))
    return cols, rows


def required_memory(n_frames: int, dim_size, window_size, overlap, search_area_size=None,
                    dtype=np.uint8, with_planes: bool = False, sliding_blocks: int = 0) -> int:
    """HBM bytes one fused call on ``n_frames`` frames needs (frames + four result planes).

    The reference's figure is the host RAM of the materialised window stack + correlation volume
    (x3.9 .. x14.8 of the frames); the fused kernel materialises neither.

    ``sliding_blocks``: the blocks of a sliding ensemble's WHOLE run (:func:`sliding_outputs`); its block store stays in HBM next
    to every chunk (:func:`sliding_store_bytes`).
    """
    sa = window_size if search_area_size is None else search_area_size
    code = _lib.DTYPE_CODES[np.dtype(dtype)]
    r = _lib.load().lspiv_required_bytes(n_frames, dim_size[0], dim_size[1], code, sa[0], sa[1],
                                         overlap[0], overlap[1], int(with_planes))
    need = _lib.check(r)
    if sliding_blocks:
        need += sliding_store_bytes(sliding_blocks, dim_size, sa, overlap)
    return need


def sliding_spec(ensemble_corr: bool, ensemble_window, ensemble_stride):
    """The sliding-ensemble keywords of ``get_ffpiv`` checked -> None (no ``ensemble_window``) or ``(M, s)`` pairs: 1 <= s <= M and
    M % s == 0; ``ensemble_stride`` None means s = M (block ensembles).  Both keywords need ``ensemble_corr=True``.  Host-only."""
    if ensemble_window is None:
        if ensemble_stride is not None:
            raise ValueError("ensemble_stride needs ensemble_window")
        return None
    if not ensemble_corr:
        raise ValueError("ensemble_window / ensemble_stride need ensemble_corr=True")
    for name, val in (("ensemble_window", ensemble_window), ("ensemble_stride", ensemble_stride)):
        if val is not None and (isinstance(val, bool) or not isinstance(val, (int, np.integer))):
            raise ValueError(f"{name} must be a whole number of frame pairs, got {val!r}")
    M = int(ensemble_window)
    s = M if ensemble_stride is None else int(ensemble_stride)
    if not (1 <= s <= M) or M % s != 0:
        raise ValueError(f"need 1 <= ensemble_stride <= ensemble_window and ensemble_window % ensemble_stride == 0, got "
                         f"ensemble_window {M}, ensemble_stride {s}")
    return M, s


def sliding_outputs(n_pairs: int, M: int, s: int) -> Tuple[int, int]:
    """(n_blk, n_out) of a sliding ensemble over ``n_pairs`` pairs: block b = pairs [b s, (b + 1) s), output j = blocks j .. j + M / s - 1.
    Trailing pairs that fill no block enter no output."""
    n_blk = n_pairs // s
    n_out = n_blk - M // s + 1
    if n_out < 1:
        raise ValueError(f"ensemble_window {M} needs at least {M} pairs, got {n_pairs}")
    return n_blk, n_out


def sliding_store_bytes(n_blocks: int, dim_size, window_size, overlap) -> int:
    """HBM bytes of a sliding ensemble's block store: one float32 plane sum and one count per (block, window).  Host-only."""
    n_rows, n_cols = get_array_shape(dim_size, window_size, overlap)
    return int(n_blocks) * n_rows * n_cols * (int(window_size[0]) * int(window_size[1]) + 1) * 4


def available_memory() -> int:
    """Free HBM on the current device in bytes (library workspaces counted as reusable)."""
    free, total = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().lspiv_available_bytes(C.byref(free), C.byref(total)))
    return free.value


def available_host_memory() -> int:
    """Free host RAM in bytes -- what ``ffpiv.window.available_memory`` answers in the reference (pyorc/velocimetry/ffpiv.py:129), and
    what bounds how much of a LAZY stack ``get_ffpiv`` may materialise at a time (the chunks that ``.load()`` brings in live on the
    host before they cross PCIe).  ``psutil`` when importable, ``/proc/meminfo`` otherwise."""
    try:
        import psutil

        return int(psutil.virtual_memory().available)
    except Exception:
        try:
            with open("/proc/meminfo") as fh:
                for line in fh:
                    if line.startswith("MemAvailable:"):
                        return int(line.split()[1]) * 1024
        except OSError:
            pass
    return 8 << 30   # nothing to ask: a conservative 8 GiB


def chunk_alignment(window_size, dim_size=None, overlap=None) -> int:
    """Frame pairs between two anchors of the time-walking kernels: time chunks that start on a multiple of it reproduce the
    whole-stack result bit for bit.  1 for per-pair kernels.  Host-only.

    The anchor length depends on the window GRID since round 5 (25 pairs; 75 on grids with at least as many windows as the chip has
    lane groups, ``lspiv_chunk_alignment_grid``): pass the frame shape ``dim_size`` and the ``overlap`` whenever chunks of frames of
    that shape are cut.  Without them the alignment that is right on EVERY grid comes back (``lspiv_chunk_alignment``, ABI 5: the
    longest anchor length of the window family, a multiple of every grid's -- 75 where ABI 4 answered 25)."""
    lib = _lib.load()
    if isinstance(window_size, SearchWindow):
        return 1   # the search-area kernels are per-pair: any chunking gives the same bits
    if dim_size is None:
        return _lib.check(lib.lspiv_chunk_alignment(int(window_size[0]), int(window_size[1])))
    ov = (int(window_size[0]) // 2, int(window_size[1]) // 2) if overlap is None else overlap
    return _lib.check(lib.lspiv_chunk_alignment_grid(int(dim_size[0]), int(dim_size[1]), int(window_size[0]), int(window_size[1]),
                                                     int(ov[0]), int(ov[1])))


def chunk_alignment_any_grid(window_size) -> int:
    """The alignment that is right for EVERY frame shape (= ``chunk_alignment(window_size)`` since ABI 5).  For callers that cut the time
    axis before they know the frames (``shard.sharded_piv`` without ``frame_shape``)."""
    return chunk_alignment(window_size)
