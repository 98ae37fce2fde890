"""Strided-batch plans (include/fft_wgpu_amd_strided.h): the columns of row-major matrices, transformed in place.

``src`` holds ``batch`` matrices of ``fft_len`` rows x ``howmany`` columns back to back; every column becomes its own DFT
over the rows -- ``numpy.fft.fft(x.reshape(batch, fft_len, howmany), axis=1)`` -- in one launch and one pass over memory.
The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse`` (``X(device, queue, src, fft_len, howmany)``,
``X.proc(encoder) -> Buffer``); the result is always ``src`` itself.

The ctypes table of the ``fws_`` functions lives here.  ``libfft_wgpu_amd_strided.so`` is loaded on first use, not when
the package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_strided.so")
ABI_VERSION = 1   # FWS_ABI_VERSION of the include/fft_wgpu_amd_strided.h this binding was written against

_P = ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
_I32 = ctypes.c_int32
_PI32 = ctypes.POINTER(_I32)

_SIGNATURES = {
    "fws_abi_version": (_I32, []),
    "fws_describe": (_I32, [_U32, _U64, _U64, _PI32, _PI32, _PI32, ctypes.POINTER(_U64)]),
    "fws_plan_create": (_I32, [_P, _I32, _U32, _U64, _P, _PP]),
    "fws_plan_exec": (_I32, [_P, _P]),
    "fws_plan_get_i64": (_I32, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "fws_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_strided.so (once).  Raises if it was not built or reports another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`make -C fft_wgpu_amd/strided`.  fft_wgpu_amd has no CPU fallback.")
        _ffi.lib()  # the main library first: the strided one links against it, and contexts and buffers are its handles
        L = ctypes.CDLL(LIB_PATH)
        try:
            L.fws_abi_version.restype = _I32
            L.fws_abi_version.argtypes = []
            got = int(L.fws_abi_version())
        except AttributeError:
            got = None
        if got != ABI_VERSION:
            raise RuntimeError(
                f"{LIB_PATH} reports ABI version {got}, this binding was written for version {ABI_VERSION} of "
                f"include/fft_wgpu_amd_strided.h: rebuild the library (`make -C fft_wgpu_amd/strided`) from the same tree")
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)  # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def describe(fft_len, howmany, batch=1):
    """The launch geometry a plan of this shape uses -- pure host logic, no GPU needed:
    {"tile_cols", "threads", "lds_bytes", "blocks"}."""
    tile, threads, lds, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fws_describe(fft_len, howmany, batch, ctypes.byref(tile), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(blocks)), None, "fws_describe")
    return {"tile_cols": tile.value, "threads": threads.value, "lds_bytes": lds.value, "blocks": blocks.value}


class _Plan:
    _kind = None

    def __init__(self, device, queue, src, fft_len, howmany):
        self.device = device
        self.queue = queue          # kept for signature parity with the contiguous plans; unused
        self.src = src
        self.fft_len = fft_len
        self.howmany = howmany
        self._S = lib()
        h = ctypes.c_void_p()
        st = self._S.fws_plan_create(device._h, self._kind, fft_len, howmany, src._h, ctypes.byref(h))
        _ffi.check(st, device._h, f"fws_plan_create({type(self).__name__})", device._L)
        self._h = h

    @classmethod
    def new(cls, *args):
        return cls(*args)

    def proc(self, encoder):
        """Enqueue the transform on ``encoder``; the result is in ``src``, which is returned."""
        st = self._S.fws_plan_exec(self._h, encoder._h if encoder is not None else None)
        _ffi.check(st, self.device._h, "fws_plan_exec", self.device._L)
        return self.src

    def get(self, key):
        v = ctypes.c_int64()
        _ffi.check(self._S.fws_plan_get_i64(self._h, key.encode(), ctypes.byref(v)), self.device._h, "fws_plan_get_i64",
                   self.device._L)
        return v.value

    def destroy(self):
        if self._h:
            self._S.fws_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Forward(_Plan):
    """Unnormalised forward DFT of every column."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """Inverse DFT of every column with the 1/fft_len scale fused into the last stage."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """Inverse DFT of every column, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED
