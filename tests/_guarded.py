"""Device buffers between guard elements for the GPU tests that call the C ABI (include/tbe_hip.h) directly."""
import numpy as np
import torch

GUARD = 64  # float32 elements before and after every buffer (256 B: the payload keeps the allocation's alignment)
CANARY = np.float32(-12345.5)


class Buf:
    """A device float32 array of `n` elements between two runs of GUARD canaries."""

    def __init__(self, n, init=None):
        self.n = int(n)
        host = np.full(self.n + 2 * GUARD, CANARY, dtype=np.float32)
        if init is not None:
            host[GUARD:GUARD + self.n] = np.asarray(init, dtype=np.float32).reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def all(self):
        return self.t.cpu().numpy()

    def get(self, shape=None):
        a = self.all()
        assert (a[:GUARD] == CANARY).all() and (a[GUARD + self.n:] == CANARY).all(), "guard elements overwritten"
        a = a[GUARD:GUARD + self.n]
        return a.reshape(shape) if shape is not None else a


GUARD_BYTES = 4 * GUARD
INT_CANARY = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}


class TypedBuf:
    """Buf for the integer arguments of an entry (int64 ids and feat_* arrays, uint8 flags, the int32 counter): `n`
    elements of `dtype` between two runs of GUARD_BYTES bytes of that type's canary."""

    def __init__(self, n, dtype, init=None):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.canary = self.dtype.type(INT_CANARY[self.dtype])
        self.guard = GUARD_BYTES // self.dtype.itemsize
        host = np.full(self.n + 2 * self.guard, self.canary, dtype=self.dtype)
        if init is not None:
            host[self.guard:self.guard + self.n] = np.asarray(init, dtype=self.dtype).reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + GUARD_BYTES
        assert self.ptr % 16 == 0

    def all(self):
        return self.t.cpu().numpy()

    def get(self, shape=None):
        a = self.all()
        g = self.guard
        assert (a[:g] == self.canary).all() and (a[g + self.n:] == self.canary).all(), "guard elements overwritten"
        a = a[g:g + self.n]
        return a.reshape(shape) if shape is not None else a
