"""Device memory for tests through the HIP runtime the product library itself is linked against (importing torch after the library
has initialised HIP would bring a second runtime into the process)."""
import ctypes

import numpy as np

_hip = None


def runtime():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    return _hip


class HipBuffer:
    """hipMalloc'd bytes, filled from a host array or with one byte value."""

    def __init__(self, host=None, nbytes=None, fill=None):
        hip = runtime()
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        self.ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(max(self.nbytes, 1))) == 0
        if host is not None:
            self.upload(host)
        elif fill is not None:
            assert hip.hipMemset(self.ptr, int(fill), ctypes.c_size_t(self.nbytes)) == 0

    @property
    def address(self):
        return self.ptr.value

    def upload(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        assert runtime().hipMemcpy(self.ptr, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.nbytes), 1) == 0

    def to_host(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.ptr, ctypes.c_size_t(self.nbytes), 2) == 0
        return out

    def free(self):
        if self.ptr:
            runtime().hipFree(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
