"""Framed real-input plans (include/fft_wgpu_amd_stft.h): the rfft of overlapping, windowed frames of long real signals,
out of place, in one launch -- the frames of ``torch.stft(..., center=False, onesided=True)`` or ``scipy.signal.stft``.

With ``n = fft_len`` a power of two from 2 to 4096, ``M = n // 2``, ``hop >= 1`` and ``L = signal_len >= n``: ``src`` holds
signals of ``L`` float32 back to back, a signal has ``F = 1 + (L - n) // hop`` frames, and ``dst`` receives one row per frame,
signal-major: ``numpy.fft.rfft(w * sliding_window_view(x, n, axis=-1)[:, ::hop], axis=-1)``.  ``Spectrum`` stores rows of
``M + 1`` complex64, ``Power`` rows of ``M + 1`` float32, ``re**2 + im**2`` of the same bins.  ``window`` is a buffer of ``n``
float32 or ``None`` (rectangular); it is read on every exec.  The classes mirror ``fft_wgpu_amd.real``
(``X(device, queue, src, dst, fft_len, hop, signal_len, window=None)``, ``X.proc(encoder) -> Buffer``); the result is always
``dst``, and ``src`` and ``window`` are never written.

The ctypes table of the ``fwt_`` functions lives here.  ``libfft_wgpu_amd_stft.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_stft.so")
ABI_VERSION = 1   # FWT_ABI_VERSION of the include/fft_wgpu_amd_stft.h this binding was written against
SPECTRUM, POWER = 0, 1   # FWT_SPECTRUM, FWT_POWER

_P = ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
_U64 = ctypes.c_uint64
_PU64 = ctypes.POINTER(_U64)
_U32 = ctypes.c_uint32
_I32 = ctypes.c_int32
_PI32 = ctypes.POINTER(_I32)

_SIGNATURES = {
    "fwt_abi_version": (_I32, []),
    "fwt_describe": (_I32, [_U32, _U32, _U64, _U64, _PU64, _PI32, _PI32, _PI32, _PU64]),
    "fwt_plan_create": (_I32, [_P, _I32, _U32, _U32, _U64, _P, _P, _P, _PP]),
    "fwt_plan_exec": (_I32, [_P, _P]),
    "fwt_plan_get_i64": (_I32, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "fwt_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_stft.so (once).  Raises if it was not built or reports another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`make -C fft_wgpu_amd/stft`.  fft_wgpu_amd has no CPU fallback.")
        _ffi.lib()  # the library it links against first: contexts, buffers, streams
        L = ctypes.CDLL(LIB_PATH)
        try:
            L.fwt_abi_version.restype = _I32
            L.fwt_abi_version.argtypes = []
            got = int(L.fwt_abi_version())
        except AttributeError:
            got = None
        if got != ABI_VERSION:
            raise RuntimeError(
                f"{LIB_PATH} reports ABI version {got}, this binding was written for version {ABI_VERSION} of "
                f"include/fft_wgpu_amd_stft.h: rebuild the library (`make -C fft_wgpu_amd/stft`) from the same tree")
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)  # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def describe(fft_len, hop, signal_len, signals=1):
    """What a plan of this length launches over ``signals`` signals of ``signal_len`` samples at this hop -- pure host logic,
    no GPU needed: {"frames_per_signal", "threads", "lds_bytes", "frames_per_block", "blocks"}."""
    per, threads, lds, rows, blocks = _U64(), _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fwt_describe(fft_len, hop, signal_len, signals, ctypes.byref(per), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(rows), ctypes.byref(blocks)), None, "fwt_describe")
    return {"frames_per_signal": per.value, "threads": threads.value, "lds_bytes": lds.value, "frames_per_block": rows.value,
            "blocks": blocks.value}


class _Plan:
    _output = None

    def __init__(self, device, queue, src, dst, fft_len, hop, signal_len, window=None):
        self.device = device
        self.queue = queue          # kept for signature parity with the contiguous plans; unused
        self.src = src
        self.dst = dst
        self.window = window
        self.fft_len = fft_len
        self.hop = hop
        self.signal_len = signal_len
        self._S = lib()
        h = ctypes.c_void_p()
        st = self._S.fwt_plan_create(device._h, self._output, fft_len, hop, signal_len, src._h,
                                     window._h if window is not None else None, dst._h, ctypes.byref(h))
        _ffi.check(st, device._h, f"fwt_plan_create({type(self).__name__})", device._L)
        self._h = h

    @classmethod
    def new(cls, *args, **kwargs):
        return cls(*args, **kwargs)

    def proc(self, encoder):
        """Enqueue the transform on ``encoder``; the result is in ``dst``, which is returned."""
        st = self._S.fwt_plan_exec(self._h, encoder._h if encoder is not None else None)
        _ffi.check(st, self.device._h, "fwt_plan_exec", self.device._L)
        return self.dst

    def get(self, key):
        v = ctypes.c_int64()
        _ffi.check(self._S.fwt_plan_get_i64(self._h, key.encode(), ctypes.byref(v)), self.device._h, "fwt_plan_get_i64",
                   self.device._L)
        return v.value

    def destroy(self):
        if self._h:
            self._S.fwt_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Spectrum(_Plan):
    """numpy.fft.rfft of every windowed frame: n / 2 + 1 complex64 per frame."""
    _output = SPECTRUM


class Power(_Plan):
    """re**2 + im**2 of numpy.fft.rfft of every windowed frame: n / 2 + 1 float32 per frame."""
    _output = POWER
