"""A recording stand-in for the ctypes library, for the host-only tests that pin what the Python wrappers send to it
(tests/test_pair_calls_host.py, tests/test_wrapper_calls_host.py).  No native code is loaded and no kernel is looked at.

Scalars are recorded as they are (floats rounded to 6 places, ctypes int arrays as tuples); a device pointer as ``(block index in
allocation order, byte offset)``; a host pointer as the name of the array of ``FakeLib.arrays`` it points into, or ``"host"`` for an
array the wrapper made itself; NULL as ``None``; a ``byref`` as ``"ref"``.  ``lspiv_dev_free`` is kept in ``FakeLib.freed``, not in the
list of calls: when a block is released depends on when the last Python reference goes, which is no property of the calls.
"""

import ctypes as C

import numpy as np
import pytest

from pyorc_amd import _lib, device

_QUERIES = ("lspiv_device_count", "lspiv_get_device", "lspiv_get_option", "lspiv_grid_shape")   # answered like `*_supported`, not recorded


class FakeLib:
    """Stands in for the ctypes library: every attribute is a function that records its call and returns 0."""

    def __init__(self):
        self.calls, self.blocks, self.freed, self.arrays = [], [], [], {}
        self._next = 1 << 40      # far from every host address

    def _ptr(self, p):
        v = p.value if isinstance(p, C.c_void_p) else int(p)
        if not v:
            return None
        for k, (base, size) in enumerate(self.blocks):
            if base <= v < base + size:
                return (k, v - base)
        for name, a in self.arrays.items():
            if a.ctypes.data <= v < a.ctypes.data + max(a.nbytes, 1):
                return name if v == a.ctypes.data else (name, v - a.ctypes.data)
        return "host"

    def _norm(self, a):
        if a is None:
            return None
        if isinstance(a, C.c_void_p):
            return self._ptr(a)
        if isinstance(a, C.Array):
            return tuple(a)
        if isinstance(a, (bool, np.bool_)):
            return bool(a)
        if isinstance(a, (float, np.floating)):
            return round(float(a), 6)
        if isinstance(a, (int, np.integer)):
            return int(a)
        if isinstance(a, bytes):
            return a.decode()
        return "ref"      # ctypes.byref(...)

    def __getattr__(self, name):
        def call(*args):
            if name == "lspiv_device_count":
                args[0]._obj.value = 1
            elif name == "lspiv_get_device":
                args[0]._obj.value = 0
            elif name == "lspiv_get_option":
                args[1]._obj.value = 1 if args[0] == b"norm_clip" else 0
            elif name == "lspiv_grid_shape":
                dim_y, dim_x, wy, wx, oy, ox = (int(q) for q in args[:6])
                args[6]._obj.value = 0 if dim_y < wy else (dim_y - wy) // (wy - oy) + 1
                args[7]._obj.value = 0 if dim_x < wx else (dim_x - wx) // (wx - ox) + 1
            if name.endswith("_supported"):
                return 1
            if name in _QUERIES:
                return 0
            if name == "lspiv_dev_free":
                self.freed.append(self._ptr(args[0]))
                return 0
            if name == "lspiv_dev_malloc":
                size = int(args[1])
                args[0]._obj.value = self._next
                self.blocks.append((self._next, size))
                self._next += max(1 << 20, (size + 0xfffff) & ~0xfffff)
                self.calls.append((name, "ref", size))
                return 0
            self.calls.append((name,) + tuple(self._norm(a) for a in args))
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    pool = device._Pool()
    pool.limit = 0        # no cached blocks: every DeviceFrames.empty is one lspiv_dev_malloc, every release one lspiv_dev_free
    monkeypatch.setattr(device, "_pool", pool)
    return lib
