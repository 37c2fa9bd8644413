"""Device buffers for the tests of the `_device` entry points, through the HIP runtime the library has loaded (no
second interpreter, no torch): upload numpy arrays, hand raw addresses to the library, read the results back."""
import ctypes as C

import numpy as np


class DeviceBuffers:
    def __init__(self):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
        hip = self.hip = C.CDLL(path)
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.ptrs = []

    def alloc(self, nbytes, fill=0xA5):
        """nbytes of device memory filled with a byte pattern (so that an output nobody wrote shows)"""
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(int(nbytes), 8)) == 0
        assert self.hip.hipMemset(p, fill, max(int(nbytes), 8)) == 0
        self.ptrs.append(p.value)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def free(self):
        self.sync()
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []
