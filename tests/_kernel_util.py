"""What tests/test_tail_gpu.py, tests/test_elementwise_gpu.py, tests/test_bn_gpu.py and tests/test_pool_gpu.py share: device and stream handles, uploads
that keep every bit, bit views of what comes back, the worst ratio of an error to its bound, ulps and guarded device buffers.  A plain module (no tests, no fixtures): the test files import from it by name."""
import ctypes as C

import numpy as np
import torch

from resunet_a_mltsk_keras_amd import _lib as L

U32 = 2.0 ** -23                                             # u of the derived bounds: one float32 ulp of a value in [1, 2)


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tdt(dt):
    return torch.bfloat16 if dt == L.RUA_BF16 else torch.float32


def vec(dt):
    return 8 if dt == L.RUA_BF16 else 4


def bit_dtype(dt):
    return np.uint16 if dt == L.RUA_BF16 else np.uint32


def up(a):
    """A copy of a numpy array on the device, dtype and bits kept."""
    return torch.from_numpy(np.array(a, order="C")).to(dev())


def from_bits(bits, dt):
    """CPU tensor of the storage type from its bit patterns (uint16 for bf16, uint32 for fp32)."""
    if dt == L.RUA_BF16:
        return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.float32))


def bits_of(t):
    """Bit patterns of a tensor (any device) as a numpy array of unsigned integers of the element's width."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.numpy().view(np.uint32)
    if t.dtype == torch.float64:
        return t.numpy().view(np.uint64)
    raise TypeError(t.dtype)


def worst_ratio(err, bound):
    """max err / bound; where the bound is zero the error has to be zero too (inf otherwise)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def ulp_of(ref, dt):
    """One unit in the last place of the storage type (RUA_F32 / RUA_BF16) in the binade of |ref|; the subnormal spacing below the smallest normal."""
    a = np.abs(np.asarray(ref, np.float64))
    e = np.where(a > 0, np.frexp(a)[1] - 1, -126)
    return np.ldexp(1.0, np.maximum(e, -126) - (7 if dt == L.RUA_BF16 else 23))


GUARD = 256                                                  # bytes in front of and behind a guarded buffer (a multiple of 16: the data stay aligned)
GUARD_BYTE = 0xA5


class Guarded:
    """A device buffer between two guard regions: `ptr` is the address of the data, get() returns the data as a numpy array of the dtype and shape
    it was made from and asserts that no guard byte changed.  bf16 tensors travel as their uint16 bit patterns."""

    def __init__(self, init, guard=GUARD):
        init = np.ascontiguousarray(init)
        self.dtype, self.shape, self.n, self.guard = init.dtype, init.shape, init.nbytes, guard
        host = np.full(self.n + 2 * guard, GUARD_BYTE, np.uint8)
        host[guard:guard + self.n] = init.view(np.uint8).reshape(-1)
        self.buf = torch.from_numpy(host).to(dev())
        self.ptr = self.buf.data_ptr() + guard

    def get(self):
        h, g = self.buf.cpu().numpy(), self.guard
        assert (h[:g] == GUARD_BYTE).all() and (h[g + self.n:] == GUARD_BYTE).all(), "a guard region changed"
        return h[g:g + self.n].view(self.dtype).reshape(self.shape).copy()


def frozen(*arrays):
    """Shared references stay as they were computed: numpy arrays made read-only."""
    for a in arrays:
        a.flags.writeable = False
    return arrays
