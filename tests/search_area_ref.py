"""Float64 numpy reference of the extended search area ("Extended search area"): an n x n window of frame t
searched inside the S x S area of frame t+1.  Composed of the oracle's own pieces (normalize_intensity, get_rect_coordinates,
signal_mask*, u_v_displacement), which it leaves as they are.  Like the rest of the PIV path it is this project's reading:
unpinned against a real ffpiv."""
import warnings

import numpy as np

from oracle import piv_oracle as po


def search_planes(imgs, window, search_area, overlap, signal_threshold=None):
    """(x, y, planes): planes (T-1, n_win, S, S) float64, NaN for pairs below the signal threshold."""
    imgs = np.asarray(imgs)
    (S, n), T = (search_area[0], window[0]), imgs.shape[0]
    o = (S - n) // 2
    x, y = po.get_rect_coordinates(imgs.shape[-2:], window, overlap, search_area_size=search_area)
    tiles = po.sliding_window_stack(imgs, search_area, overlap)          # the grid of the search area: (T, n_win, S, S)
    blocks = tiles[..., o:o + n, o:o + n]
    planes = np.full((T - 1,) + tiles.shape[1:], np.nan)
    keep_pos = po.signal_mask_stack(tiles, signal_threshold) if po.SEMANTICS["signal_mode"] == 1 else None
    for t in range(T - 1):
        # the window's fraction over n^2, the search area's over S^2 (signal_mask scores a pair: each window paired with itself)
        keep = (po.signal_mask(blocks[t], blocks[t], signal_threshold) & po.signal_mask(tiles[t + 1], tiles[t + 1], signal_threshold)
                if keep_pos is None else keep_pos)
        A = np.zeros(tiles.shape[1:])
        A[:, o:o + n, o:o + n] = po.normalize_intensity(blocks[t])
        B = po.normalize_intensity(tiles[t + 1])
        c = np.fft.irfft2(np.conj(np.fft.rfft2(A)) * np.fft.rfft2(B), s=(S, S))
        c = np.clip(np.fft.fftshift(c, axes=(-2, -1)) / float(n * n), 0.0, 1.0)
        planes[t, keep] = c[keep]
    return x, y, planes


def search_piv(imgs, window, search_area, overlap, signal_threshold=None):
    """dict(u, v, corr, s2n (T-1, n_rows, n_cols), planes, tie): ``tie`` marks the windows whose arg-max is a matter of rounding in
    any implementation -- an exact float64 tie for the plane maximum, which includes the clip at 1 binding on two samples."""
    x, y, planes = search_planes(imgs, window, search_area, overlap, signal_threshold)
    n_rows, n_cols = len(y), len(x)
    shape = (planes.shape[0], n_rows, n_cols)
    u, v = po.u_v_displacement(planes, n_rows, n_cols)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN planes (windows below the signal threshold)
        cm = np.nanmax(planes, axis=(-2, -1))
        s2n = cm / np.nanmean(planes, axis=(-2, -1))
    top = np.sort(planes.reshape(planes.shape[:2] + (-1,)), axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        tie = ((top[..., 1] - top[..., 0]) <= 1e-12 * top[..., 1]) & (cm > 0)
    return dict(u=u, v=v, corr=cm.reshape(shape), s2n=s2n.reshape(shape), planes=planes, tie=tie.reshape(shape), x=x, y=y)
