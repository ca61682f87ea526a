"""What tests/test_tail_gpu.py and tests/test_elementwise_gpu.py share: device and stream handles, uploads that keep every bit, bit views
of what comes back, and the worst ratio of an error to its bound.  A plain module (no tests, no fixtures): the test files import from it by name."""
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


def frozen(*arrays):
    """Shared references stay as they were computed: numpy arrays made read-only."""
    for a in arrays:
        a.flags.writeable = False
    return arrays
