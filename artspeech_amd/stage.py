"""What the packed-audio stages share (join, master, marks, mimic, resample and the library calls of vocoder): two array rules behind one
interface, the stage's device, the keyed workspace cache and the sample outputs.

A stage fills its C I/O struct in ONE function that takes a rule: ``Device(dev)`` for the call on the GPU, ``Host()`` for the ``*_host``
twin.  A rule checks or normalises an input (``need``, ``values_i32``; None passes through), gives an array's address (``at``; None: NULL)
and its element count (``count``), and allocates ``empty`` / ``zeros`` where it lives.  Dtypes are named as torch names them on both sides.
"""
import numpy as np
import torch

from . import _lib

I32, F32, I16, U8 = torch.int32, torch.float32, torch.int16, torch.uint8


class Device:
    """Tensors on one GPU.  `need` refuses; it never converts, copies or reads: a call through it stays capturable."""
    __slots__ = ("dev",)
    names = {I32: "int32", F32: "float32"}
    at = staticmethod(_lib.ptr)
    count = staticmethod(torch.Tensor.numel)

    def __init__(self, dev):
        self.dev = dev

    def need(self, t, dtype, what, name, vector=False):
        """t, a contiguous tensor (vector: of one axis) of `dtype` on a GPU, or None; `what: name` is how the refusal calls it"""
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (vector and t.dim() != 1)):
            raise ValueError(f"{what}: {name} must be a contiguous {self.names[dtype]} {'vector' if vector else 'tensor'} on the GPU")
        return t

    def values_i32(self, v, n, what, name):
        """n int32 values: a list is uploaded here, a device vector is taken as it is (and the call stays capturable)"""
        if v is None:
            return None
        if not torch.is_tensor(v):
            v = torch.tensor(list(v), dtype=I32).to(self.dev)
        if v.dtype != I32 or not v.is_cuda or not v.is_contiguous() or v.numel() != n:
            raise ValueError(f"{what}: {name} must be {n} int32 values (a list, or a contiguous vector on the GPU)")
        return v

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.dev)


class Host:
    """numpy arrays: whatever converts is taken (what, name, vector and n serve the device rule alone)"""
    _np = {I32: np.int32, F32: np.float32, I16: np.int16, U8: np.uint8}
    count = staticmethod(np.size)

    def need(self, a, dtype, what=None, name=None, vector=False):
        return None if a is None else np.ascontiguousarray(a, self._np[dtype])

    def values_i32(self, v, n=None, what=None, name=None):
        return self.need(v, I32)

    @staticmethod
    def at(a):
        return None if a is None else a.ctypes.data

    def empty(self, shape, dtype):
        return np.empty(shape, self._np[dtype])

    def zeros(self, shape, dtype):
        return np.zeros(shape, self._np[dtype])


_GPU = False


def device(dev=None):
    """the GPU a stage runs on: `dev` where it names one, else the current device; without a GPU there is nothing to run on"""
    global _GPU
    if not _GPU:                                # (asked until there is one: a process does not lose its GPU)
        _GPU = torch.cuda.is_available()
        if not _GPU:
            raise _lib.HipLibraryError("the HIP path needs a GPU: torch.cuda.is_available() is False (no CPU fallback)")
    if dev is None or dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class Workspaces:
    """(device, key) -> uint8 tensor: the SAME tensor at every call with the same key, as a captured graph needs"""

    def __init__(self):
        self._ws = {}

    def get(self, dev, key, nbytes, error):
        """nbytes(): the bytes the library asks for (asked once per key); 0 bytes: ValueError with the caller's text `error`"""
        key = (dev.index,) + key
        ws = self._ws.get(key)
        if ws is None:
            n = nbytes()
            if n == 0:
                raise ValueError(error)
            ws = self._ws[key] = torch.empty(n, dtype=U8, device=dev)
        return ws


def samples(rule, n, wav, pcm, what="forward_packed", lead=()):
    """the sample outputs of a stage -> (y fp32 lead + [n] or None, p16 int16 [n] or None)"""
    if not (wav or pcm):
        raise ValueError(f"{what}: at least one of wav and pcm")
    return rule.empty(lead + (n,), F32) if wav else None, rule.empty(n, I16) if pcm else None
