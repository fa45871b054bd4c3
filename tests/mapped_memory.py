"""Mapped pinned host memory for the tests that hand it to an entry point as an output (a numpy / ctypes helper module, as
tests/route_model.py): include/se3tracknet.h admits it wherever it says "device memory or mapped pinned host memory"."""
import ctypes as C

import numpy as np


class Mapped:
    """mapped pinned host memory from the HIP runtime the library runs on: .d is the address the device reaches it by"""

    def __init__(self, nbytes):
        self.hip, self.nbytes = C.CDLL(None), nbytes
        self.h, self.d = C.c_void_p(), C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(self.h), C.c_size_t(nbytes), C.c_uint(2)) == 0          # hipHostMallocMapped
        assert self.hip.hipHostGetDevicePointer(C.byref(self.d), self.h, C.c_uint(0)) == 0
        C.memset(self.h, 0xEE, nbytes)

    def read(self):
        return np.frombuffer(C.string_at(self.h, self.nbytes), np.uint8).copy()

    def close(self):
        self.hip.hipHostFree(self.h)
