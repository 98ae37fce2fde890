"""Real-input plans (include/fft_wgpu_amd_real.h): rfft and irfft of batched rows, out of place, in one launch.

With ``n = fft_len`` a power of two from 2 to 4096 and ``M = n // 2``: ``Forward`` takes ``src`` -- ``batch`` rows of ``n``
float32 -- to ``dst`` -- ``batch`` rows of ``M + 1`` complex64, ``numpy.fft.rfft(x, axis=-1)``; ``Onlyinverse`` takes
``batch`` rows of ``M + 1`` complex64 to ``batch`` rows of ``n`` float32, ``n * numpy.fft.irfft(X, n, axis=-1)``, and
``Inverse`` is ``numpy.fft.irfft`` itself.  The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse``
(``X(device, queue, src, dst, fft_len)``, ``X.proc(encoder) -> Buffer``); the result is always ``dst``, and ``src`` is
never written.

The ctypes table of the ``fwr_`` functions lives here.  ``libfft_wgpu_amd_real.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_real.so")
ABI_VERSION = 1   # FWR_ABI_VERSION of the include/fft_wgpu_amd_real.h this binding was written against

_P = ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
_I32 = ctypes.c_int32
_PI32 = ctypes.POINTER(_I32)

_SIGNATURES = {
    "fwr_abi_version": (_I32, []),
    "fwr_describe": (_I32, [_U32, _U64, _PI32, _PI32, _PI32, ctypes.POINTER(_U64)]),
    "fwr_plan_create": (_I32, [_P, _I32, _U32, _P, _P, _PP]),
    "fwr_plan_exec": (_I32, [_P, _P]),
    "fwr_plan_get_i64": (_I32, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "fwr_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_real.so (once).  Raises if it was not built or reports another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`make -C fft_wgpu_amd/real`.  fft_wgpu_amd has no CPU fallback.")
        _ffi.lib()  # the library it links against first: contexts, buffers, streams
        L = ctypes.CDLL(LIB_PATH)
        try:
            L.fwr_abi_version.restype = _I32
            L.fwr_abi_version.argtypes = []
            got = int(L.fwr_abi_version())
        except AttributeError:
            got = None
        if got != ABI_VERSION:
            raise RuntimeError(
                f"{LIB_PATH} reports ABI version {got}, this binding was written for version {ABI_VERSION} of "
                f"include/fft_wgpu_amd_real.h: rebuild the library (`make -C fft_wgpu_amd/real`) from the same tree")
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)  # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def describe(fft_len, batch=1):
    """What a plan of this length over ``batch`` rows launches -- pure host logic, no GPU needed:
    {"threads", "lds_bytes", "rows_per_block", "blocks"}."""
    threads, lds, rows, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fwr_describe(fft_len, batch, ctypes.byref(threads), ctypes.byref(lds), ctypes.byref(rows),
                                  ctypes.byref(blocks)), None, "fwr_describe")
    return {"threads": threads.value, "lds_bytes": lds.value, "rows_per_block": rows.value, "blocks": blocks.value}


class _Plan:
    _kind = None

    def __init__(self, device, queue, src, dst, fft_len):
        self.device = device
        self.queue = queue          # kept for signature parity with the contiguous plans; unused
        self.src = src
        self.dst = dst
        self.fft_len = fft_len
        self._S = lib()
        h = ctypes.c_void_p()
        st = self._S.fwr_plan_create(device._h, self._kind, fft_len, src._h, dst._h, ctypes.byref(h))
        _ffi.check(st, device._h, f"fwr_plan_create({type(self).__name__})", device._L)
        self._h = h

    @classmethod
    def new(cls, *args):
        return cls(*args)

    def proc(self, encoder):
        """Enqueue the transform on ``encoder``; the result is in ``dst``, which is returned."""
        st = self._S.fwr_plan_exec(self._h, encoder._h if encoder is not None else None)
        _ffi.check(st, self.device._h, "fwr_plan_exec", self.device._L)
        return self.dst

    def get(self, key):
        v = ctypes.c_int64()
        _ffi.check(self._S.fwr_plan_get_i64(self._h, key.encode(), ctypes.byref(v)), self.device._h, "fwr_plan_get_i64",
                   self.device._L)
        return v.value

    def destroy(self):
        if self._h:
            self._S.fwr_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Forward(_Plan):
    """numpy.fft.rfft of every row: n float32 -> n / 2 + 1 complex64."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """numpy.fft.irfft of every row: n / 2 + 1 complex64 -> n float32."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """n * numpy.fft.irfft of every row, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED
