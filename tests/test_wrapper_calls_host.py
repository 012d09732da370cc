"""What the wrappers of ``pyorc_amd.stabilize``, ``pyorc_amd.stiv`` and ``pyorc_amd.track`` send to the library, pinned call by call, in
the style of tests/test_pair_calls_host.py and with its recording fake (tests/fake_lib.py has the notation).  Host-only.

Every case runs one public call on a 4-frame 24 x 40 uint8 stack, as a host array and as a ``DeviceFrames`` (block 0 of its trace; a
device-side ``out`` or space-time image of the case is block 1), and compares the list of library calls it made with a literal below.

The literals were generated from the wrappers of the PARENT commit -- when ``stabilize.py`` still held ``_device_buffer`` and
``_download`` and every module its own stack and ``out`` checks -- and the folded code has to reproduce them.  ``lspiv_dev_free`` is
left out of the compared list; instead every block a case allocates must have been freed exactly once at its end.  The fake returns
zeros and fills nothing, so what ``estimate`` reads back is arbitrary and its identity-pair ``RuntimeWarning`` may fire: it is filtered.
"""

import gc
import warnings

import numpy as np
import pytest

from pyorc_amd import device, stabilize, stiv, track
from tests.fake_lib import fake  # noqa: F401  (the fixture)

T, H, W = 4, 24, 40
P, N, S, L = T - 1, 3, 2, 9


def _arrays():
    return {"imgs": np.zeros((T, H, W), np.uint8), "A": np.tile(np.eye(2, 3), (T, 1, 1)), "mask": np.ones((H, W), bool),
            "carry": np.eye(2, 3), "lines": np.array([[1.0, 2.0, 30.0, 2.0], [5.0, 1.0, 5.0, 20.0]]),
            "sti_out": np.zeros((S, T + 3, L), np.float32), "sti": np.zeros((S, T, L), np.float32),
            "points": np.array([[3.0, 4.0], [20.5, 11.25], [39.0, 23.0]]), "guess": np.zeros((P, N, 2))}


def _side(r, name, dev):
    """Array ``name`` of the case on the stack's side: itself, or a ``DeviceFrames`` of its shape."""
    return device.DeviceFrames.empty(r[name].shape, r[name].dtype) if dev else r[name]


CASES = {
    "warp": lambda s, r, dev: stabilize.warp(s, r["A"]),
    "estimate": lambda s, r, dev: stabilize.estimate(s, r["mask"], window_size=16),
    "estimate_carry": lambda s, r, dev: stabilize.estimate(s, r["mask"], window_size=16, model="affine", carry=r["carry"]),
    "sti": lambda s, r, dev: stiv.space_time_images(s, r["lines"], L),
    "sti_out": lambda s, r, dev: stiv.space_time_images(s, r["lines"], L, out=_side(r, "sti_out", dev), t_offset=2),
    "orientation": lambda s, r, dev: stiv.orientation(_side(r, "sti", dev), time_window=3, time_stride=1, smooth=0),
    "pyr_down": lambda s, r, dev: track.pyr_down(s),
    "track_pairs": lambda s, r, dev: track.track_pairs(s, r["points"], window=5, levels=2, guess=r["guess"]),
    "trajectories": lambda s, r, dev: track.trajectories(s, r["points"], window=7, levels=2, max_iter=5),
}
KINDS = ("host", "dev")


def trace_of(lib, case, kind):
    r = _arrays()
    lib.arrays = r
    dev = kind == "dev"
    stack = device.DeviceFrames.empty((T, H, W), np.uint8) if dev else r["imgs"]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = CASES[case](stack, r, dev)
    del stack, res
    gc.collect()
    return lib.calls


# ---- the expected traces (see the module's docstring) ----------------------------------------------------------------------------------
_FIT = (3, 2, 4, 16, 8, 8, 24, 40)      # pairs, the grid of 16 px windows at overlap 8, the frame
EXPECTED = {
    ('estimate', 'host'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 0, 4, 24, 40, 16, 16, 8, 8, 'host', 128, -1.0, 0, 'host', 'host', 'host', 'host', None),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (0, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_stabilize_fit_dev', (0, 0), (1, 0), *_FIT, 1, 2.0, 0.5, 6, (2, 0), (3, 0), None),
        ('lspiv_stabilize_chain_dev', (2, 0), 3, None, (4, 0), (5, 0), None),
        ('lspiv_memcpy_d2h', 'host', (4, 0), 192),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 144),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 12),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 48),
    ],
    ('estimate', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 1024),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 960),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_masked_pairs_dev_at', (0, 0), 0, 4, 24, 40, 16, 16, 8, 8, (1, 0), 128, -1.0, 0, (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 384),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (3, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (4, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_stabilize_fit_dev', (3, 0), (4, 0), *_FIT, 1, 2.0, 0.5, 6, (5, 0), (6, 0), None),
        ('lspiv_stabilize_chain_dev', (5, 0), 3, None, (7, 0), (8, 0), None),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 192),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 144),
        ('lspiv_memcpy_d2h', 'host', (6, 0), 12),
        ('lspiv_memcpy_d2h', 'host', (8, 0), 48),
    ],
    ('estimate_carry', 'host'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 0, 4, 24, 40, 16, 16, 8, 8, 'host', 128, -1.0, 0, 'host', 'host', 'host', 'host', None),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (0, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (6, 0), 'carry', 48),
        ('lspiv_stabilize_fit_dev', (0, 0), (1, 0), *_FIT, 2, 2.0, 0.5, 6, (2, 0), (3, 0), None),
        ('lspiv_stabilize_chain_dev', (2, 0), 3, (6, 0), (4, 0), (5, 0), None),
        ('lspiv_memcpy_d2h', 'host', (4, 0), 192),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 144),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 12),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 48),
    ],
    ('estimate_carry', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 1024),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 960),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_masked_pairs_dev_at', (0, 0), 0, 4, 24, 40, 16, 16, 8, 8, (1, 0), 128, -1.0, 0, (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 384),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (3, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (4, 0), 'host', 96),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (9, 0), 'carry', 48),
        ('lspiv_stabilize_fit_dev', (3, 0), (4, 0), *_FIT, 2, 2.0, 0.5, 6, (5, 0), (6, 0), None),
        ('lspiv_stabilize_chain_dev', (5, 0), 3, (9, 0), (7, 0), (8, 0), None),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 192),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 144),
        ('lspiv_memcpy_d2h', 'host', (6, 0), 12),
        ('lspiv_memcpy_d2h', 'host', (8, 0), 48),
    ],
    ('orientation', 'host'): [
        ('lspiv_sti_orientation', 'sti', 2, 4, 9, 3, 1, 0, 1, 'host', 'host', 'host'),
    ],
    ('orientation', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_sti_orientation_dev', (1, 0), 2, 4, 9, 3, 1, 0, 1, (2, 0), (3, 0), (4, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 96),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 32),
        ('lspiv_memcpy_d2h', 'host', (4, 0), 32),
    ],
    ('pyr_down', 'host'): [
        ('lspiv_pyr_down', 'imgs', 0, 4, 24, 40, 'host'),
    ],
    ('pyr_down', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_pyr_down_dev', (0, 0), 0, 4, 24, 40, (1, 0), None),
    ],
    ('sti', 'host'): [
        ('lspiv_sti_gather', 'imgs', 0, 4, 24, 40, 'host', 2, 9, 'host', 0, 4),
    ],
    ('sti', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_sti_gather_dev', (0, 0), 0, 4, 24, 40, 'host', 2, 9, (1, 0), 0, 4, None),
    ],
    ('sti_out', 'host'): [
        ('lspiv_sti_gather', 'imgs', 0, 4, 24, 40, 'host', 2, 9, 'sti_out', 2, 7),
    ],
    ('sti_out', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_sti_gather_dev', (0, 0), 0, 4, 24, 40, 'host', 2, 9, (1, 0), 2, 7, None),
    ],
    ('track_pairs', 'host'): [
        ('lspiv_lk_track', 'imgs', 0, 4, 24, 40, 'points', 3, 0, 'guess', 1, 5, 2, 20, 0.01, 0.0, 0, 'host', 'host', 'host', 'host', 'host', 'host', None),
    ],
    ('track_pairs', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (1, 0), 'points', 48),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (2, 0), 'guess', 144),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_lk_track_dev', (0, 0), 0, 4, 24, 40, (1, 0), 3, 0, (2, 0), 1, 5, 2, 20, 0.01, 0.0, 0, (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (4, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (6, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 36),
        ('lspiv_memcpy_d2h', 'host', (8, 0), 9),
    ],
    ('trajectories', 'host'): [
        ('lspiv_lk_track', 'imgs', 0, 4, 24, 40, 'points', 3, 0, None, 0, 7, 2, 5, 0.01, 0.0, 1, 'host', 'host', 'host', 'host', 'host', 'host', 'host'),
    ],
    ('trajectories', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (1, 0), 'points', 48),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_lk_track_dev', (0, 0), 0, 4, 24, 40, (1, 0), 3, 0, None, 0, 7, 2, 5, 0.01, 0.0, 1, (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (4, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 72),
        ('lspiv_memcpy_d2h', 'host', (6, 0), 36),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 9),
        ('lspiv_memcpy_d2h', 'host', (8, 0), 192),
    ],
    ('warp', 'host'): [
        ('lspiv_warp_affine', 'imgs', 0, 4, 24, 40, 'A', 'host'),
    ],
    ('warp', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 3840),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (2, 0), 'A', 192),
        ('lspiv_warp_affine_dev', (0, 0), 0, 4, 24, 40, (2, 0), (1, 0), None),
    ],
}  # end of EXPECTED


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_calls(fake, case, kind):
    got = trace_of(fake, case, kind)
    assert got == EXPECTED[case, kind]
    assert sorted(fake.freed) == [(k, 0) for k in range(len(fake.blocks))]      # every block freed, once
