"""Plumbing shared by the engine's wrapper modules (every section of include/ngcf_hip.h takes device pointers and a stream): pointers,
the current device and stream, scratch, views over library-owned memory - tuned to the microsecond, they run a dozen times per
training step - and the argument checks that several set-up and evaluation families state in the same words."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch


def _require_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on '{t.device}': the NGCF propagation engine runs on a ROCm device only "
            "(hand-written HIP kernels, no CPU/PyTorch fallback). Move the module and inputs to 'cuda'.")


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    _require_device(t, what)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {t.dtype}")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_NULL = contextlib.nullcontext()


def _on(device):
    """`torch.cuda.device(device)`, or nothing at all when that device is already current (the context manager costs ~8 us per
    use, a dozen times per forward on a launch-bound graph)."""
    dev = torch.device(device)
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NULL
    return torch.cuda.device(dev)


def _stream():
    """torch's current stream on the current device as a hipStream_t.  (The raw getter where this torch has it: the Stream
    object of `torch.cuda.current_stream()` costs ~8 us to build, seven times per forward on a launch-bound graph.)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _row_major_ld(t: torch.Tensor, what: str) -> int:
    """Leading dimension of a 2-D row-major (possibly column-sliced) fp32 tensor."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{what}: expected a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


class Workspace:
    """A grow-only byte buffer on one device, handed to the kernels as scratch."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf


class _DevView:
    """`__cuda_array_interface__` carrier over library-owned device memory."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(n),), "typestr": typestr, "version": 2}


def _device_view(ptr: int, n: int, dtype, device=None) -> torch.Tensor:
    """A torch tensor over `n` elements of library-owned memory on `device` (None: the current one); no copy, the owner must outlive it."""
    if ptr == 0:
        raise RuntimeError("null device pointer")
    return torch.as_tensor(_DevView(ptr, n, {torch.int64: "<i8", torch.int32: "<i4", torch.float32: "<f4"}[dtype]),
                           device=torch.device("cuda", torch.cuda.current_device()) if device is None else device)


# ---- argument checks shared by the set-up and evaluation wrappers: plain functions that raise ------------------------------------
# `fn` is the wrapper's name as its messages spell it, `pairs` are (argument name, tensor or None) and a None is not checked.
def _status_word(fn: str, status: Optional[torch.Tensor], dev):
    """`(word, read_back)`: the caller's int32 word on `dev`, which the wrapper leaves to them, or a fresh zeroed one to read back."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=dev), True
    if status.dtype != torch.int32 or status.device != dev:
        raise ValueError(f"{fn}: status must be an int32 tensor on {dev}")
    return status, False


def _sums_slots(fn: str, sums: Optional[torch.Tensor], n_slots: int, dev, exc=ValueError) -> torch.Tensor:
    """The caller's float64 slot vector to add into, or a fresh zeroed one."""
    if sums is None:
        return torch.zeros(n_slots, dtype=torch.float64, device=dev)
    if sums.dtype != torch.float64 or sums.numel() != n_slots or sums.device != dev or not sums.is_contiguous():
        raise exc(f"{fn}: sums must be a contiguous float64 tensor of {n_slots} slots on {dev}")
    return sums


def _unit_inner(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """`t` as it is when its inner stride is 1 (a slice of a table's rows or columns), a contiguous copy otherwise."""
    return t if t is None or t.stride(1) == 1 else t.contiguous()


def _seed_array(seeds):
    """The cumulative 64-bit layer seeds of node dropout as the `const uint64_t *` the library takes (never of length 0)."""
    return (C.c_uint64 * max(len(seeds), 1))(*[int(x) & (2 ** 64 - 1) for x in seeds])


def _require_dtype(fn: str, dtype, pairs):
    """Every tensor of `pairs` has `dtype`."""
    for nm, t in pairs:
        if t is not None and t.dtype != dtype:
            raise TypeError(f"{fn}: {nm} must be {str(dtype).split('.')[-1]}, got {t.dtype}")


def _require_same_device(fn: str, pairs, anchor: str, dev):
    """Every tensor of `pairs` lives on `dev`, the device of the argument `anchor`."""
    for nm, t in pairs:
        if t is not None and t.device != dev:
            raise RuntimeError(f"{fn}: {nm} is on {t.device}, {anchor} on {dev}")


def _require_matmul(a: torch.Tensor, b: torch.Tensor):
    """`a @ b.T` exists: torch.mm's own words for two row tables whose widths differ."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(a.shape)} and {tuple(b.t().shape)})")
