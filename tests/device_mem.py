"""Plain device memory for the export tests: hipMalloc / hipMemset / hipFree of the HIP runtime libp264amd.so itself is linked
against (reached through the library's handle, so that the process holds ONE runtime), and the library's own synchronous copies."""
import ctypes as C

import numpy as np


class DeviceBuffer:
    def __init__(self, lib, nbytes, fill=0xA5):
        self.lib, self.nbytes = lib, int(nbytes)
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        lib.hipFree.argtypes = [C.c_void_p]
        p = C.c_void_p()
        assert lib.hipMalloc(C.byref(p), max(self.nbytes, 1)) == 0
        self.ptr = p.value
        self.fill(fill)

    def fill(self, value):
        assert self.lib.hipMemset(self.ptr, value, self.nbytes) == 0
        assert self.lib.hipDeviceSynchronize() == 0

    def host(self):
        out = np.empty(self.nbytes, np.uint8)
        assert self.lib.p264hip_copy_from_device(out.ctypes.data, self.ptr, self.nbytes) == 0
        return out

    def free(self):
        if self.ptr:
            self.lib.hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
