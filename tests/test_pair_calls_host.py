"""What the per-pair PIV wrappers of ``pyorc_amd.piv`` send to the library, pinned call by call.  Host-only: ``_lib.load`` is replaced
by a recording fake (tests/fake_lib.py), no native code is loaded and no kernel is looked at.

Every case runs one public call on a 4-frame 96 x 112 stack (host uint8, host float64, ``DeviceFrames``) and compares the list of
library calls it made -- name and arguments -- with a literal below.  Scalars are recorded as they are (floats rounded to 6 places,
ctypes int arrays as tuples); a device pointer as ``(block index in allocation order, byte offset)``; a host pointer as the name of
the array of the case it points into, or ``"host"`` for an array the wrapper made itself; NULL as ``None``; a ``byref`` as ``"ref"``.
``lspiv_memcpy_*`` carry their byte counts, so a wrong result-block offset shows, not only a wrong scalar.

The literals were generated from the wrappers as they stood BEFORE the host layer was folded into one driver, and the folded code has
to reproduce them.  ``lspiv_dev_free`` is left out of the compared list (when a block is released depends on when the last Python
reference goes, which is no property of the calls); instead every block a case allocates must have been freed exactly once at its end.
The order of the ``lspiv_dev_malloc`` calls is kept as it was, so the block indices need no translation into roles.
"""

import gc

import numpy as np
import pytest

from pyorc_amd import device, piv, window
from tests.fake_lib import fake  # noqa: F401  (the fixture)

T, H, W = 4, 96, 112
P = T - 1
GRID = (5, 6)        # 32 px windows at overlap 16 on 96 x 112


def _arrays(kind):
    r = {"imgs": np.zeros((T, H, W), np.float64 if kind == "f64" else np.uint8),
         "dt": np.full(P, 0.04), "mask": np.ones((H, W), bool),
         "shift": np.zeros((P,) + GRID + (2,), np.int16), "nodes": np.zeros((P,) + GRID + (2,), np.int32)}
    for k in range(4):
        r[f"out{k}"] = np.zeros((P,) + GRID, np.float32)
    return r


W32, O16 = (32, 32), (16, 16)
CHAIN = [(64, 32), (32, 16)]
CASES = {
    "plain": lambda s, r: piv.piv_pairs(s, W32, O16, 0.1, return_planes=True, pair_offset=25),
    "scale": lambda s, r: piv.piv_pairs(s, W32, O16, scale=(0.01, 0.02, r["dt"])),
    "out": lambda s, r: piv.piv_pairs(s, W32, O16, out=[r[f"out{k}"] for k in range(4)]),
    "search": lambda s, r: piv.piv_pairs(s, (12, 12), O16, search_area_size=(32, 32)),
    "search_scale": lambda s, r: piv.piv_pairs(s, (12, 12), O16, search_area_size=(32, 32), scale=(0.01, 0.02, r["dt"])),
    "search_planes": lambda s, r: piv.piv_pairs(s, (12, 12), O16, 0.1, return_planes=True, pair_offset=25, search_area_size=(32, 32)),
    "filtered": lambda s, r: piv.piv_pairs_filtered(s, (16, 16), (8, 8)),
    "filtered_planes": lambda s, r: piv.piv_pairs_filtered(s, (16, 16), (8, 8), "spof", 0.1, True, 25),
    "masked": lambda s, r: piv.piv_pairs_masked(s, W32, O16, r["mask"]),
    "masked_out_scale": lambda s, r: piv.piv_pairs_masked(s, W32, O16, r["mask"], 0.5, out=[r[f"out{k}"] for k in range(4)],
                                                           scale=(0.01, 0.02, r["dt"])),
    "shifted": lambda s, r: piv.piv_pairs_shifted(s, W32, O16),
    "shifted_shift": lambda s, r: piv.piv_pairs_shifted(s, W32, O16, r["shift"], 0.1, True, 25),
    "deformed": lambda s, r: piv.piv_pairs_deformed(s, W32, O16),
    "deformed_nodes": lambda s, r: piv.piv_pairs_deformed(s, W32, O16, r["nodes"], 0.1, True, 25),
    "multipass_shift": lambda s, r: piv.piv_multipass(s, CHAIN, return_shift=True),
    "multipass_deform": lambda s, r: piv.piv_multipass(s, CHAIN, 0.1, True, 25, deform_passes=1),
    "multipass_passes": lambda s, r: piv.piv_multipass(s, CHAIN, return_passes=True),
    "route_multipass": lambda s, r: piv.piv_pairs(s, window.MultiPassWindow(CHAIN, 1), O16, out=[r[f"out{k}"] for k in range(4)],
                                                  scale=(0.01, 0.02, r["dt"])),
    "route_filtered": lambda s, r: piv.piv_pairs(s, window.FilteredWindow((16, 16), "spof"), (8, 8), 0.1, pair_offset=25),
    "route_masked": lambda s, r: piv.piv_pairs(s, window.MaskedWindow(W32, r["mask"], 0.25), O16, return_planes=True),
}
KINDS = ("u8", "f64", "dev")


def trace_of(lib, case, kind):
    """The calls of one case; the stack of a ``dev`` case is block 0."""
    r = _arrays(kind)
    lib.arrays = r
    stack = device.DeviceFrames.empty((T, H, W), np.uint8) if kind == "dev" else r["imgs"]
    with np.errstate(all="ignore"):
        res = CASES[case](stack, r)
    del stack, res
    gc.collect()
    return lib.calls


# ---- the expected traces (see the module's docstring) ----------------------------------------------------------------------------------
EXPECTED = {
    ('deformed', 'u8'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_upload_frames', (0, 0), 'imgs', 0, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (1, 0), (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
    ],
    ('deformed', 'f64'): [
        ('lspiv_dev_malloc', 'ref', 180224),
        ('lspiv_upload_frames', (0, 0), 'imgs', 2, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 1, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (1, 0), (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
    ],
    ('deformed', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (1, 0), (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
    ],
    ('deformed_nodes', 'u8'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_upload_frames', (0, 0), 'imgs', 0, 4, 96, 112, 0.1),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'nodes', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('deformed_nodes', 'f64'): [
        ('lspiv_dev_malloc', 'ref', 180224),
        ('lspiv_upload_frames', (0, 0), 'imgs', 2, 4, 96, 112, 0.1),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'nodes', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 1, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('deformed_nodes', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 768),
        ('lspiv_memcpy_h2d', (1, 0), 'nodes', 720),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_deform_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('filtered', 'u8'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 0, 4, 96, 112, 16, 16, 8, 8, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('filtered', 'f64'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 2, 4, 96, 112, 16, 16, 8, 8, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('filtered', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 7168),
        ('lspiv_piv_spof_pairs_dev_at', (0, 0), 0, 4, 96, 112, 16, 16, 8, 8, -1.0, 0, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 6864),
    ],
    ('filtered_planes', 'u8'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 0, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('filtered_planes', 'f64'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 2, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('filtered_planes', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 7168),
        ('lspiv_dev_malloc', 'ref', 458752),
        ('lspiv_piv_spof_pairs_dev_at', (0, 0), 0, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, (1, 0), (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 6864),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 439296),
    ],
    ('masked', 'u8'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, 'host', 256, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('masked', 'f64'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, 'host', 256, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('masked', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 11264),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 10752),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_masked_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, (1, 0), 256, -1.0, 0, (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
    ],
    ('masked_out_scale', 'u8'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, 'host', 512, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None),
    ],
    ('masked_out_scale', 'f64'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, 'host', 512, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None),
    ],
    ('masked_out_scale', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 11264),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 10752),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_masked_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, (1, 0), 512, -1.0, 0, (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'out0', (2, 0), 360),
        ('lspiv_memcpy_d2h', 'out1', (2, 360), 360),
        ('lspiv_memcpy_d2h', 'out2', (2, 720), 360),
        ('lspiv_memcpy_d2h', 'out3', (2, 1080), 360),
    ],
    ('multipass_deform', 'u8'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_piv_multipass_deform_at', 'imgs', 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, 0.1, 25, 'host', 'host', 'host', 'host', 'host',
         None),
    ],
    ('multipass_deform', 'f64'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_piv_multipass_deform_at', 'imgs', 2, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, 0.1, 25, 'host', 'host', 'host', 'host', 'host',
         None),
    ],
    ('multipass_deform', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, 0.1, 25, (1, 0), (2, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 368640),
    ],
    ('multipass_passes', 'u8'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_upload_frames', (0, 0), 'imgs', 0, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, (1, 0), None, (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 360),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_piv_pairs_dev_at', (0, 0), 0, 4, 96, 112, 64, 64, 32, 32, -1.0, 0, (3, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 192),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (4, 0), 'host', 48),
        ('lspiv_memcpy_h2d', (4, 48), 'host', 48),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_predict_shift_dev', (4, 0), (4, 48), 3, 96, 112, 64, 64, 32, 32, 32, 32, 16, 16, (5, 0), None),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 360),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (6, 0), 'host', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (6, 0), (7, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 1440),
    ],
    ('multipass_passes', 'f64'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_dev_malloc', 'ref', 180224),
        ('lspiv_upload_frames', (0, 0), 'imgs', 2, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 1, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, (1, 0), None, (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 360),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_piv_pairs_dev_at', (0, 0), 1, 4, 96, 112, 64, 64, 32, 32, -1.0, 0, (3, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 192),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (4, 0), 'host', 48),
        ('lspiv_memcpy_h2d', (4, 48), 'host', 48),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_predict_shift_dev', (4, 0), (4, 48), 3, 96, 112, 64, 64, 32, 32, 32, 32, 16, 16, (5, 0), None),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 360),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (6, 0), 'host', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 1, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (6, 0), (7, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 1440),
    ],
    ('multipass_passes', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, (1, 0), None, (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 360),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_piv_pairs_dev_at', (0, 0), 0, 4, 96, 112, 64, 64, 32, 32, -1.0, 0, (3, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 192),
        ('lspiv_dev_malloc', 'ref', 256),
        ('lspiv_memcpy_h2d', (4, 0), 'host', 48),
        ('lspiv_memcpy_h2d', (4, 48), 'host', 48),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_predict_shift_dev', (4, 0), (4, 48), 3, 96, 112, 64, 64, 32, 32, 32, 32, 16, 16, (5, 0), None),
        ('lspiv_memcpy_d2h', 'host', (5, 0), 360),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (6, 0), 'host', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (6, 0), (7, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (7, 0), 1440),
    ],
    ('multipass_shift', 'u8'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_piv_multipass_deform_at', 'imgs', 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, 'host', 'host', 'host', 'host', None,
         'host'),
    ],
    ('multipass_shift', 'f64'): [
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_piv_multipass_deform_at', 'imgs', 2, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, 'host', 'host', 'host', 'host', None,
         'host'),
    ],
    ('multipass_shift', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_kernel_kind', 64, 64),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 0, -1.0, 0, (1, 0), None, (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 360),
    ],
    ('out', 'u8'): [
        ('lspiv_piv_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None),
    ],
    ('out', 'f64'): [
        ('lspiv_piv_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None),
    ],
    ('out', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'out0', (1, 0), 360),
        ('lspiv_memcpy_d2h', 'out1', (1, 360), 360),
        ('lspiv_memcpy_d2h', 'out2', (1, 720), 360),
        ('lspiv_memcpy_d2h', 'out3', (1, 1080), 360),
    ],
    ('plain', 'u8'): [
        ('lspiv_piv_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('plain', 'f64'): [
        ('lspiv_piv_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('plain', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 368640),
    ],
    ('route_filtered', 'u8'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 0, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, 'host', 'host', 'host', 'host', None),
    ],
    ('route_filtered', 'f64'): [
        ('lspiv_piv_spof_pairs_at', 'imgs', 2, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, 'host', 'host', 'host', 'host', None),
    ],
    ('route_filtered', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 7168),
        ('lspiv_piv_spof_pairs_dev_at', (0, 0), 0, 4, 96, 112, 16, 16, 8, 8, 0.1, 25, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 6864),
    ],
    ('route_masked', 'u8'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, 'host', 256, -1.0, 0, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('route_masked', 'f64'): [
        ('lspiv_piv_masked_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, 'host', 256, -1.0, 0, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('route_masked', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 11264),
        ('lspiv_memcpy_h2d', (1, 0), 'host', 10752),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_masked_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, (1, 0), 256, -1.0, 0, (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('route_multipass', 'u8'): [
        ('lspiv_piv_multipass_deform_at', 'imgs', 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None, None),
    ],
    ('route_multipass', 'f64'): [
        ('lspiv_piv_multipass_deform_at', 'imgs', 2, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, -1.0, 0, 'out0', 'out1', 'out2', 'out3', None, None),
    ],
    ('route_multipass', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_multipass_deform_dev_at', (0, 0), 0, 4, 96, 112, 2, (64, 64, 32, 32, 32, 32, 16, 16), 1, -1.0, 0, (1, 0), None, None, None),
        ('lspiv_memcpy_d2h', 'out0', (1, 0), 360),
        ('lspiv_memcpy_d2h', 'out1', (1, 360), 360),
        ('lspiv_memcpy_d2h', 'out2', (1, 720), 360),
        ('lspiv_memcpy_d2h', 'out3', (1, 1080), 360),
    ],
    ('scale', 'u8'): [
        ('lspiv_piv_velocity_at', 'imgs', 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, 0.01, 0.02, 'dt', 'host', 'host', 'host', 'host'),
    ],
    ('scale', 'f64'): [
        ('lspiv_piv_velocity_at', 'imgs', 2, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, 0.01, 0.02, 'dt', 'host', 'host', 'host', 'host'),
    ],
    ('scale', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, (1, 0), None, None),
        ('lspiv_scale_velocity_dev', (1, 0), 3, 30, 0.01, 0.02, 'dt', None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('search', 'u8'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('search', 'f64'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('search', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_search_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('search_planes', 'u8'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('search_planes', 'f64'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 12, 12, 16, 16, 0.1, 25, 'host', 'host', 'host', 'host', 'host'),
    ],
    ('search_planes', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_search_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, 0.1, 25, (1, 0), (2, 0), None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 368640),
    ],
    ('search_scale', 'u8'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('search_scale', 'f64'): [
        ('lspiv_piv_search_pairs_at', 'imgs', 2, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, 'host', 'host', 'host', 'host', None),
    ],
    ('search_scale', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_search_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 12, 12, 16, 16, -1.0, 0, (1, 0), None, None),
        ('lspiv_scale_velocity_dev', (1, 0), 3, 30, 0.01, 0.02, 'dt', None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('shifted', 'u8'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_upload_frames', (0, 0), 'imgs', 0, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, None, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('shifted', 'f64'): [
        ('lspiv_dev_malloc', 'ref', 180224),
        ('lspiv_upload_frames', (0, 0), 'imgs', 2, 4, 96, 112, -1.0),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 1, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, None, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('shifted', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, -1.0, 0, None, (1, 0), None, None),
        ('lspiv_memcpy_d2h', 'host', (1, 0), 1440),
    ],
    ('shifted_shift', 'u8'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_upload_frames', (0, 0), 'imgs', 0, 4, 96, 112, 0.1),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (1, 0), 'shift', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('shifted_shift', 'f64'): [
        ('lspiv_dev_malloc', 'ref', 180224),
        ('lspiv_upload_frames', (0, 0), 'imgs', 2, 4, 96, 112, 0.1),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (1, 0), 'shift', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 1, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
    ('shifted_shift', 'dev'): [
        ('lspiv_dev_malloc', 'ref', 45056),
        ('lspiv_dev_malloc', 'ref', 512),
        ('lspiv_memcpy_h2d', (1, 0), 'shift', 360),
        ('lspiv_dev_malloc', 'ref', 1536),
        ('lspiv_dev_malloc', 'ref', 393216),
        ('lspiv_piv_shift_pairs_dev_at', (0, 0), 0, 4, 96, 112, 32, 32, 16, 16, 0.1, 25, (1, 0), (2, 0), (3, 0), None),
        ('lspiv_memcpy_d2h', 'host', (2, 0), 1440),
        ('lspiv_memcpy_d2h', 'host', (3, 0), 368640),
    ],
}  # end of EXPECTED


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_calls(fake, case, kind):
    got = trace_of(fake, case, kind)
    assert got == EXPECTED[case, kind]
    assert sorted(fake.freed) == [(k, 0) for k in range(len(fake.blocks))]      # every block freed, once


def test_masked_k_min_of_an_all_true_mask(fake):
    calls = trace_of(fake, "masked", "u8")
    (c,) = [c for c in calls if c[0] == "lspiv_piv_masked_pairs_at"]
    assert c[11] == 256      # max(2, ceil(0.25 * 32 * 32))


SPECS = {"coarse_passes": lambda r: window.MultiPassWindow(CHAIN), "spectral_filter": lambda r: window.FilteredWindow(W32, "spof"),
         "image_mask": lambda r: window.MaskedWindow(W32, r["mask"])}


@pytest.mark.parametrize("keyword", sorted(SPECS))
def test_search_area_with_a_mode_spec_is_refused(fake, keyword):
    r = _arrays("u8")
    with pytest.raises(NotImplementedError, match=f"^{keyword} together with a search_area_size larger than the window is not implemented$"):
        piv.piv_pairs(r["imgs"], SPECS[keyword](r), O16, search_area_size=(64, 64))
    assert not [c for c in fake.calls if "_pairs" in c[0] or "multipass" in c[0]]
    # a search area equal to the window is today's path of the mode
    piv.piv_pairs(r["imgs"], SPECS[keyword](r), O16, search_area_size=W32)
    assert [c for c in fake.calls if "_pairs" in c[0] or "multipass" in c[0]]


SCALED = {
    "piv_pairs": lambda s, r, **kw: piv.piv_pairs(s, W32, O16, **kw),
    "search": lambda s, r, **kw: piv.piv_pairs(s, (12, 12), O16, search_area_size=W32, **kw),
    "filtered": lambda s, r, **kw: piv.piv_pairs_filtered(s, W32, O16, **kw),
    "masked": lambda s, r, **kw: piv.piv_pairs_masked(s, W32, O16, r["mask"], **kw),
    "multipass": lambda s, r, **kw: piv.piv_multipass(s, CHAIN, **kw),
}  # end of SCALED


@pytest.mark.parametrize("kind", ("u8", "dev"))
@pytest.mark.parametrize("mode", sorted(SCALED))
def test_scale_excludes_return_planes(fake, mode, kind):
    r = _arrays(kind)
    stack = device.DeviceFrames.empty((T, H, W), np.uint8) if kind == "dev" else r["imgs"]
    with pytest.raises(ValueError, match="^scale and return_planes exclude each other$"):
        SCALED[mode](stack, r, return_planes=True, scale=(0.01, 0.02, r["dt"]))
    with pytest.raises(ValueError, match=r"^scale: dt must have one entry per frame pair \(3\), got shape \(2,\)$"):
        SCALED[mode](stack, r, scale=(0.01, 0.02, r["dt"][:2]))
    assert not [c for c in fake.calls if "_pairs" in c[0] or "multipass" in c[0] or "velocity" in c[0]]


@pytest.mark.parametrize("res", ((0.01, 0.02), (np.float64(0.01), np.float64(0.02))), ids=("float", "float64"))
@pytest.mark.parametrize("mode,kind", [(m, k) for m in sorted(SCALED) for k in ("u8", "dev")
                                       if m != "piv_pairs" and (m, k) != ("search", "dev")])     # (those two scale on the device)
def test_host_scaling_is_numpys(fake, mode, kind, res):
    """The modes without a fused scaling entry point scale on the host: ``(u * res / dt).astype(float32)`` as numpy computes it (the
    product in numpy's type for that resolution, the division in float64, one rounding).  The fake library writes nothing, so the
    caller's ``out`` arrays keep what the test put there and come back scaled."""
    r = _arrays(kind)
    rng = np.random.default_rng(7)
    px = [rng.standard_normal((P,) + GRID).astype(np.float32) * 5 for _ in range(4)]
    out = [q.copy() for q in px]
    dt = np.array([0.04, 0.05, 0.03])
    stack = device.DeviceFrames.empty((T, H, W), np.uint8) if kind == "dev" else r["imgs"]
    got = SCALED[mode](stack, r, out=out, scale=(res[0], res[1], dt))
    assert all(g is o for g, o in zip(got, out))
    for k in range(2):
        assert np.array_equal(got[k], (px[k] * res[k] / dt[:, None, None]).astype(np.float32))
    for k in (2, 3):
        assert np.array_equal(got[k], px[k])
    assert not [c for c in fake.calls if c[0] in ("lspiv_scale_velocity_dev", "lspiv_piv_velocity_at")]
