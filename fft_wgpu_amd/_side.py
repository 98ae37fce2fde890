"""What the plan classes of the side libraries (strided, fft2d, real, conv, stft) share: one handle of ``<prefix>_plan`` behind
``new / proc / get / destroy``.  A subclass names its ``_prefix`` and builds the handle with ``_create``; the C calls are the
library's ``<prefix>_plan_create / _exec / _get_i64 / _destroy``.  There is no fallback: a failing call raises.
"""
import ctypes

from . import _ffi


class Plan:
    _prefix = None  # "fws", "fw2", ...

    def _create(self, L, device, queue, result, *args):
        """``<prefix>_plan_create(*args, &handle)`` on the loaded library ``L``; ``result`` is the buffer ``proc`` returns."""
        self.device = device
        self.queue = queue          # kept for signature parity with the contiguous plans; unused
        self._S = L
        self._result = result
        h = ctypes.c_void_p()
        st = self._call("create", *args, ctypes.byref(h))
        _ffi.check(st, device._h, f"{self._prefix}_plan_create({type(self).__name__})", device._L)
        self._h = h

    def _call(self, what, *args):
        return getattr(self._S, f"{self._prefix}_plan_{what}")(*args)

    @classmethod
    def new(cls, *args, **kwargs):
        return cls(*args, **kwargs)

    def proc(self, encoder):
        """Enqueue one exec on ``encoder``; returns the buffer that holds the result (``src`` of an in-place plan, else ``dst``)."""
        st = self._call("exec", self._h, encoder._h if encoder is not None else None)
        _ffi.check(st, self.device._h, f"{self._prefix}_plan_exec", self.device._L)
        return self._result

    def get(self, key):
        v = ctypes.c_int64()
        _ffi.check(self._call("get_i64", self._h, key.encode(), ctypes.byref(v)), self.device._h, f"{self._prefix}_plan_get_i64",
                   self.device._L)
        return v.value

    def destroy(self):
        if self._h:
            self._call("destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
