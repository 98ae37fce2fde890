"""2-D plans (include/fft_wgpu_amd_2d.h): batched row-major images, transformed in place.

``src`` holds ``batch`` images of ``rows`` x ``cols`` back to back; a plan computes
``numpy.fft.fft2(x.reshape(batch, rows, cols))`` (``ifft2`` for the inverses) in one launch (rows, cols <= 32) or two, for
every power-of-two width and height from 2 to 4096.  The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse``
(``X(device, queue, src, rows, cols)``, ``X.proc(encoder) -> Buffer``); the result is always ``src`` itself.

The ctypes table of the ``fw2_`` functions lives here.  ``libfft_wgpu_amd_2d.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi
from . import strided as _strided

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_2d.so")
ABI_VERSION = 1   # FW2_ABI_VERSION of the include/fft_wgpu_amd_2d.h this binding was written against

_P = ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
_I32 = ctypes.c_int32
_PI32 = ctypes.POINTER(_I32)

_SIGNATURES = {
    "fw2_abi_version": (_I32, []),
    "fw2_describe": (_I32, [_U32, _U32, _U64, _PI32, _PI32, _PI32, ctypes.POINTER(_U64)]),
    "fw2_plan_create": (_I32, [_P, _I32, _U32, _U32, _P, _PP]),
    "fw2_plan_exec": (_I32, [_P, _P]),
    "fw2_plan_get_i64": (_I32, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "fw2_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_2d.so (once).  Raises if it was not built or reports another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`make -C fft_wgpu_amd/fft2d`.  fft_wgpu_amd has no CPU fallback.")
        _strided.lib()  # the libraries it links against first: the main one (contexts, buffers) and the column plans
        L = ctypes.CDLL(LIB_PATH)
        try:
            L.fw2_abi_version.restype = _I32
            L.fw2_abi_version.argtypes = []
            got = int(L.fw2_abi_version())
        except AttributeError:
            got = None
        if got != ABI_VERSION:
            raise RuntimeError(
                f"{LIB_PATH} reports ABI version {got}, this binding was written for version {ABI_VERSION} of "
                f"include/fft_wgpu_amd_2d.h: rebuild the library (`make -C fft_wgpu_amd/fft2d`) from the same tree")
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)  # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def describe(rows, cols, batch=1):
    """What a plan of this shape launches -- pure host logic, no GPU needed:
    {"launches", "row_threads", "row_lds_bytes", "row_blocks"}."""
    launches, threads, lds, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fw2_describe(rows, cols, batch, ctypes.byref(launches), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(blocks)), None, "fw2_describe")
    return {"launches": launches.value, "row_threads": threads.value, "row_lds_bytes": lds.value, "row_blocks": blocks.value}


class _Plan:
    _kind = None

    def __init__(self, device, queue, src, rows, cols):
        self.device = device
        self.queue = queue          # kept for signature parity with the contiguous plans; unused
        self.src = src
        self.rows = rows
        self.cols = cols
        self._S = lib()
        h = ctypes.c_void_p()
        st = self._S.fw2_plan_create(device._h, self._kind, rows, cols, src._h, ctypes.byref(h))
        _ffi.check(st, device._h, f"fw2_plan_create({type(self).__name__})", device._L)
        self._h = h

    @classmethod
    def new(cls, *args):
        return cls(*args)

    def proc(self, encoder):
        """Enqueue the transform on ``encoder``; the result is in ``src``, which is returned."""
        st = self._S.fw2_plan_exec(self._h, encoder._h if encoder is not None else None)
        _ffi.check(st, self.device._h, "fw2_plan_exec", self.device._L)
        return self.src

    def get(self, key):
        v = ctypes.c_int64()
        _ffi.check(self._S.fw2_plan_get_i64(self._h, key.encode(), ctypes.byref(v)), self.device._h, "fw2_plan_get_i64",
                   self.device._L)
        return v.value

    def destroy(self):
        if self._h:
            self._S.fw2_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Forward(_Plan):
    """Unnormalised forward 2-D DFT of every image."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """Inverse 2-D DFT of every image, scaled by 1 / (rows * cols)."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """Inverse 2-D DFT of every image, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED
