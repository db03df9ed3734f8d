"""The optimizer of the reference's training loop on the device: `optim.Adam` replaces the `torch.optim.Adam` that main.py:74 builds
and experiment.py:58 steps.  One kernel launch per 32 parameters updates p, exp_avg and exp_avg_sq and advances the step counters
(`engine.optim.adam_step`, csrc/adam.hip; include/ngcf_hip.h holds the recipe operation by operation, tests/adam_oracle.py restates it
on the host, and the kernel is pinned to that bit for bit).

Against torch's Adam: the same update - no amsgrad, weight decay added to the gradient - but not torch's bits: those depend on how
torch's element-wise kernels were compiled and on the host's `pow`.  One step from equal state lies within a few units in the last
place of torch's (tools/adam_lab.py measures it, tests/test_adam_gpu.py holds it); over a training run such differences compound, as
they do between two builds of torch."""
from __future__ import annotations

import torch

from . import engine as _eng

_GROUP_DEFAULTS = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": True, "differentiable": False, "fused": None,
                   "decoupled_weight_decay": False}
_REFUSED = ("amsgrad", "decoupled_weight_decay", "differentiable")


def _refuse_tensor(name, value):
    if isinstance(value, torch.Tensor):
        raise TypeError(f"optim.Adam: a tensor `{name}` is not supported: the launch takes {name} as a Python float")


class Adam(torch.optim.Optimizer):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay, maximize=...)` as one HIP launch per 32 parameters and param group.

    A `torch.optim.Optimizer`: param groups, `zero_grad`, `state_dict` and hooks are torch's.  State per parameter, created on its
    first step with a gradient, is torch's key set and layout: `step` (a 0-dim float32 tensor on the device, exact up to 2^24 steps),
    `exp_avg`, `exp_avg_sq`.  Every param group says `capturable=True` - the step counters live on the device and the kernel advances
    them - so `GraphedTrainStep` and `torch.cuda.graph` take the optimizer as it is, and a `state_dict` goes to and from a
    `torch.optim.Adam(..., capturable=True)`.  A float `lr` (and betas, eps, weight_decay) is baked into a captured step, exactly as
    torch's float `lr` is: change it, capture again.

    A parameter whose `.grad` is None is left out of the step: its value, state and step counter stay as they are.  A gradient that
    is not contiguous is made so first; a parameter that is not contiguous is an error.  Parameters are float32 and on a ROCm device
    when `step()` runs; the parameters of one group share a device.

    Refused with an error that names the option: `amsgrad`, `decoupled_weight_decay`, `differentiable`, a tensor `lr` (or beta),
    sparse gradients, parameters that are not float32, parameters on the CPU, a grad scaler's `found_inf` / `grad_scale`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, maximize=False):
        for name, value in (("lr", lr), ("betas[0]", betas[0]), ("betas[1]", betas[1]), ("eps", eps), ("weight_decay", weight_decay)):
            _refuse_tensor(name, value)
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_GROUP_DEFAULTS)
        defaults["maximize"] = maximize
        super().__init__(params, defaults)

    # ---- what is refused -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group):
        for name in _REFUSED:
            if group.get(name, False):
                raise NotImplementedError(f"optim.Adam: `{name}` is not supported (torch.optim.Adam has it)")
        for name in ("lr", "eps", "weight_decay"):
            _refuse_tensor(name, group[name])
        for k in (0, 1):
            _refuse_tensor(f"betas[{k}]", group["betas"][k])

    @staticmethod
    def _check_param_dtype(p):
        if p.dtype != torch.float32:      # complex included
            raise TypeError(f"optim.Adam: a parameter of dtype {p.dtype} is not supported: float32 only")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                self._check_param_dtype(p)
        except Exception:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        """Unpickling and `load_state_dict`: groups written by a torch.optim.Adam get this class's flags, and a step counter that
        torch kept on the host (capturable=False) moves to its parameter's device."""
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in _GROUP_DEFAULTS.items():
                group.setdefault(k, v)
            group["capturable"] = True
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    step = st["step"]
                    if not torch.is_tensor(step):
                        step = torch.tensor(float(step), dtype=torch.float32)
                    if step.device != p.device or step.dtype != torch.float32 or step.dim() != 0:
                        st["step"] = step.detach().to(device=p.device, dtype=torch.float32).reshape(())

    # ---- device words ----------------------------------------------------------------------------------------------------------------
    def _new_step(self, device):
        """A zeroed 0-dim step counter: a view of one buffer per device, so the counters of a model sit in one allocation."""
        bufs = self.__dict__.setdefault("_step_bufs", {})
        buf, used = bufs.get(device, (None, 0))
        if buf is None or used == buf.numel():
            buf, used = torch.zeros(max(sum(len(g["params"]) for g in self.param_groups), 1), dtype=torch.float32, device=device), 0
        bufs[device] = (buf, used + 1)
        return buf[used]

    def _ticket(self, device):
        tickets = self.__dict__.setdefault("_tickets", {})
        if device not in tickets:
            tickets[device] = _eng.optim.new_ticket(device)
        return tickets[device]

    # ---- the step --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """One optimization step; `closure`, if given, re-evaluates the model under grad mode and its loss is returned."""
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for name in ("found_inf", "grad_scale"):
            if getattr(self, name, None) is not None:
                raise NotImplementedError(f"optim.Adam: a grad scaler's `{name}` is not supported: unscale and skip outside the optimizer")
        for group in self.param_groups:
            self._check_group(group)
            params, grads, exp_avgs, exp_avg_sqs, steps = [], [], [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("optim.Adam: sparse gradients are not supported (torch has SparseAdam for them)")
                self._check_param_dtype(p)
                if not p.is_cuda:
                    raise NotImplementedError(f"optim.Adam: a parameter on '{p.device}' is not supported: the step is a HIP kernel, there "
                                              "is no CPU path. Move the module to 'cuda', or use torch.optim.Adam")
                if not p.is_contiguous():
                    raise ValueError(f"optim.Adam: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not contiguous")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = self._new_step(p.device)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                params.append(p)
                grads.append(g if g.is_contiguous() else g.contiguous())
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                steps.append(state["step"])
            if params:
                _eng.optim.adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, self._ticket(params[0].device), lr=group["lr"],
                                     betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"],
                                     maximize=group["maximize"])
        return loss
