"""The optimizer step of the training loop: `ngcf_adam_step_f32` (csrc/adam.hip; the header's section "Adam step" holds the recipe,
operation by operation).  Reached as `engine.optim.<name>`; `seoul_tourism_recommendation_ngcf_amd.optim.Adam` is the optimizer
built on it."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_dtype, _require_same_device, _stream

ADAM_MAX_TENSORS = 32       # NGCF_ADAM_MAX_TENSORS: tensors of one launch
ADAM_CHUNK = 4096           # elements of one workgroup


def new_ticket(device) -> torch.Tensor:
    """The zeroed device word that the launches of one optimizer count their workgroups in."""
    return torch.zeros(1, dtype=torch.int32, device=device)


def adam_step(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
              exp_avg_sqs: Sequence[torch.Tensor], steps: Sequence[torch.Tensor], ticket: torch.Tensor, *, lr: float,
              betas: Tuple[float, float], eps: float, weight_decay: float, maximize: bool) -> None:
    """One Adam step of every tensor in place, torch.optim.Adam's update (no amsgrad, weight decay added to the gradient): one launch
    per 32 tensors, asynchronous on the current stream, capturable as it stands.  `params[i]`, `grads[i]`, `exp_avgs[i]`,
    `exp_avg_sqs[i]`: float32, contiguous, of one shape, on one device; an empty tensor is skipped.  `steps[i]`: a float32 tensor of
    one element on that device, the steps taken so far - torch's capturable format; the kernel advances it, exactly up to 2^24 steps.
    The step tensors must not share memory.  `ticket`: `new_ticket(device)`, the same word for every call of one optimizer, 0 between
    calls.  `lr`, `betas`, `eps`, `weight_decay` are Python floats and are baked into a captured launch.  Equal inputs give equal
    bits on every run; the bits are those of tests/adam_oracle.py."""
    lib = _lib.load()
    fn = "adam_step"
    lists = (("params", params), ("grads", grads), ("exp_avgs", exp_avgs), ("exp_avg_sqs", exp_avg_sqs), ("steps", steps))
    n = len(params)
    for nm, ts in lists:
        if len(ts) != n:
            raise ValueError(f"{fn}: {len(ts)} {nm} for {n} params")
        for i, t in enumerate(ts):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{fn}: {nm}[{i}] is not a tensor")
    for name, value in (("lr", lr), ("betas[0]", betas[0]), ("betas[1]", betas[1]), ("eps", eps), ("weight_decay", weight_decay)):
        if isinstance(value, torch.Tensor):
            raise TypeError(f"{fn}: {name} must be a Python float, not a tensor")
    if not isinstance(ticket, torch.Tensor) or ticket.dtype != torch.int32 or ticket.numel() != 1:
        raise TypeError(f"{fn}: ticket must be an int32 tensor of one element")
    if n == 0:
        return
    _require_dtype(fn, torch.float32, [(f"{nm}[{i}]", t) for nm, ts in lists for i, t in enumerate(ts)])
    _require_device(params[0], "params[0]")
    dev = params[0].device
    _require_same_device(fn, [(f"{nm}[{i}]", t) for nm, ts in lists for i, t in enumerate(ts)] + [("ticket", ticket)], "params[0]", dev)
    for i in range(n):
        shape = params[i].shape
        for nm, ts in lists[:4]:
            if ts[i].shape != shape:
                raise ValueError(f"{fn}: {nm}[{i}] has shape {tuple(ts[i].shape)}, params[{i}] {tuple(shape)}")
            if not ts[i].is_contiguous():
                raise ValueError(f"{fn}: {nm}[{i}] must be contiguous")
        if steps[i].numel() != 1:
            raise ValueError(f"{fn}: steps[{i}] must hold one element, got shape {tuple(steps[i].shape)}")
    ptrs = [(C.c_void_p * n)(*[t.data_ptr() for t in ts]) for _, ts in lists]
    numel = (C.c_int64 * n)(*[t.numel() for t in params])
    with _on(dev):
        _lib.check(lib.ngcf_adam_step_f32(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], numel, _ptr(ticket), float(lr), float(betas[0]),
                                          float(betas[1]), float(eps), float(weight_decay), int(bool(maximize)), _stream()))
