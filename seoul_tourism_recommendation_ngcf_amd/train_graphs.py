"""`NGCF.auto_train_graph`: the training forward and its backward, captured on the second call of a shape as two hipGraphs and
replayed afterwards.

`NGCF.forward` asks `train_graph_wanted(model, ...)` and, if so, hands the call to `forward_train_graphed(model, ...)`; a None from
it means "run eagerly".  `_TrainGraphs` is the capture of one shape, `_ReplayTrain` the autograd node of a replay.  The state
stays on the model: `_train_graphs`, `_train_seen`, `_train_calls`, `_capture_warned`, `_alias`, `_forced_year_idx`.
"""
from __future__ import annotations

import warnings
import weakref
from typing import Optional

import torch

from . import engine as _eng
from .NGCF import NGCF
from .all_e import _static_result_held, static_result_baseline
from .graphed import _batch_sizes, _graph_key


class _ReplayTrain(torch.autograd.Function):
    """autograd node of a graph-replayed training forward: forward = replay of the captured forward graph, backward = replay of the
    captured backward graph; the static gradient buffers are handed to the model's parameters."""

    @staticmethod
    def forward(ctx, runner, *params):
        runner.fwd.replay()
        ctx.runner = runner
        # The saved activations live in the graphs' static pool and are shared by every replay: while this node can still run its
        # backward, a second replay would overwrite what that backward needs.  The token dies with the node (the caller dropped
        # the loss without a backward) and is dropped when the backward has run; `_TrainGraphs.outstanding()` reads it.
        ctx.token = _Token()
        runner.pending = weakref.ref(ctx.token)
        fresh = [torch.empty_like(o) for o in runner.outs]             # fresh tensors like the eager path (the graph's own are overwritten
        torch._foreach_copy_(fresh, [o.detach() for o in runner.outs])  # by the next replay): one multi-tensor copy
        return tuple(fresh)

    @staticmethod
    def backward(ctx, *grads):
        r = ctx.runner
        if ctx.token is None or r.pending is None or r.pending() is not ctx.token:
            raise RuntimeError("NGCF: this training forward was replayed from a captured graph and its saved activations have been "
                               "overwritten (a second backward through the same forward, or a replay forced in between); set "
                               "model.auto_train_graph = False for such loops")
        ctx.token, r.pending = None, None
        have = [(s, g) for s, g in zip(r.gouts, grads) if g is not None and g.data_ptr() != s.data_ptr()]
        if have:
            torch._foreach_copy_([s for s, _ in have], [g for _, g in have])      # the incoming gradients into the graph's inputs: one launch
        for s, g in zip(r.gouts, grads):
            if g is None:
                s.zero_()
        # The gradients leave as the graph's own buffers (no copies): with `zero_grad()` between two backward passes (the default
        # sets `.grad` to None) autograd adopts them and the next replay finds nobody holding them.  A `.grad` that still IS one
        # of these buffers - gradient accumulation over several backward calls, or `zero_grad(set_to_none=False)` - gets its own
        # storage first, or the replay would overwrite what it is about to be added to.
        for p, g in zip(r.params, r.gins):
            if g is not None and p.grad is not None and p.grad.data_ptr() == g.data_ptr():
                p.grad = p.grad.clone()
        r.bwd.replay()
        return (None, *[None if g is None else g.detach() for g in r.gins])


class _Token:
    """(weak-referenceable marker of an outstanding replayed forward)"""
    __slots__ = ("__weakref__",)


class _TrainGraphs:
    """`NGCF.auto_train_graph`: the eager training forward of one shape and its backward, captured as two hipGraphs that share a
    memory pool (the pattern of `torch.cuda.make_graphed_callables`, with one difference that matters here: the differentiable
    inputs of the capture are fresh ALIASES of the parameters - same storage, new leaves.  The parameters themselves carry
    AccumulateGrad nodes from earlier eager steps for as long as the caller keeps a loss tensor alive, and those belong to the
    default stream: the captured backward would wait for an event recorded outside the capture, which ends the process on this
    runtime)."""

    def __init__(self, model, year_idx: int, node_flag: bool, has_neg: bool, args):
        self.model, self.year_idx, self.node_flag, self.has_neg = model, year_idx, node_flag, has_neg
        self.flat = torch.cat(args)                                    # static index vectors: views of one buffer (one copy per call)
        self.idx, o = [], 0
        for a in args:
            self.idx.append(self.flat[o:o + a.numel()])
            o += a.numel()
        self.params = model._diff_params()
        self.pending = None
        # Both graphs bake in the addresses of everything their kernels touch.  The workspace is this object's own (the module's
        # grow-only one is re-allocated when an eager call asks for more - the other year slice, a larger batch - and the old block
        # goes back to the allocator); the module's scratch / status / seed-state tensors are long-lived, referenced here so that
        # their memory cannot be handed out again, and compared before every replay (`intact`).
        self.ws = _eng.Workspace()
        uw = model.user_embedding.weight.data
        rows_before = uw[self.idx[0].clamp(0, model.n_user - 1)].clone()   # the warm-up forwards inject for real (NGCF.py:114): undone below
        saved_ws, model._ws = model._ws, self.ws
        try:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                              # warm-up: everything lazily created exists before the capture
                for _ in range(3):
                    al = self._aliases()
                    outs = self._body(al)
                    torch.autograd.grad(outs, al, grad_outputs=[torch.empty_like(o) for o in outs], allow_unused=True)
                    del outs, al
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            pool = torch.cuda.graph_pool_handle()
            self.fwd, self.bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            al = self._aliases()
            status_host = model._status_host_buf()
            with torch.cuda.graph(self.fwd, pool=pool):
                outs = self._body(al)
                status_host.copy_(model._status, non_blocking=True)    # last node: the status word where the host can see it
            self.outs = tuple(outs)
            self.all_E = model._all_E.detach()                         # the capture's all_E: what the module's attributes alias after a replay
            self.gouts = tuple(torch.empty_like(o) for o in outs)
            with torch.cuda.graph(self.bwd, pool=pool):
                gins = torch.autograd.grad(outs, al, grad_outputs=self.gouts, allow_unused=True)
            self.gins = tuple(gins)
        finally:
            model._ws = saved_ws
        # emb_ratio != 1: the injection blends (w <- w (1-r) + feats r) and is not idempotent - the three warm-up forwards must not
        # count, or the batch's user rows would be blended four times by the time of the first replay
        uw[self.idx[0].clamp(0, model.n_user - 1)] = rows_before
        self._keep = (self.ws.buf, model._scratch, model._status, getattr(model, "_seed_state", None), model._status_host)
        self._baked = self._pointers()
        model._all_E = model.all_users_emb = model.all_items_emb = None     # (they alias the capture's all_E: set again by every replay)
        self._free = static_result_baseline(self.all_E)                      # ... which only this object and its autograd nodes hold now

    def _pointers(self):
        m = self.model
        return tuple(None if t is None else t.data_ptr() for t in (self.ws.buf, m._scratch, m._status, getattr(m, "_seed_state", None), m._status_host))

    def intact(self) -> bool:
        """Every buffer whose address the two graphs bake in is still the tensor it was at capture."""
        return self._pointers() == self._baked

    def outstanding(self) -> bool:
        """A forward replayed from these graphs can still run its backward (its saved activations must not be overwritten)."""
        return self.pending is not None and self.pending() is not None

    def _aliases(self):
        return [p.detach().requires_grad_(True) for p in self.params]

    def _body(self, aliases):
        m = self.model
        saved = (m.check_indices, m._forced_year_idx, m.auto_train_graph, m._alias)
        m.check_indices, m._forced_year_idx, m.auto_train_graph, m._alias = False, self.year_idx, False, aliases   # no host syncs inside
        try:
            u_id, age, sex, month, day, dow, pos = self.idx[:7]
            neg = self.idx[7] if self.has_neg else torch.empty(0, dtype=torch.int64)
            u, p, n = NGCF.forward(m, u_id, u_id, age, sex, month, day, dow, pos, neg, self.node_flag)
        finally:
            m.check_indices, m._forced_year_idx, m.auto_train_graph, m._alias = saved
        return (u, p, n) if self.has_neg else (u, p)

    def __call__(self, *args):
        torch.cat(args, out=self.flat)
        outs = _ReplayTrain.apply(self, *self.params)
        m = self.model
        m._e0_cache.invalidate()                                       # (the replay injected rows through `.data`)
        m._all_E = self.all_E                                          # NGCF.py:148-149: the attributes follow the forward that just ran
        m.all_users_emb, m.all_items_emb = self.all_E[:m.n_user, :], self.all_E[m.n_user:, :]
        return outs


def train_graph_wanted(model, node_flag, u_id, pos_item, neg_item) -> bool:
    """A differentiable forward of a launch-bound size whose random masks (if any) are drawn on the device.  r04: `model.training`
    is NOT required - the reference's own loop calls `self.model.eval()` at the end of its first epoch and never `train()` again
    (experiment.py:61,72), so from epoch 2 on it trains in eval mode: autograd on, `node_flag=True` (node dropout still drawn,
    NGCF.py:124-126), message dropout off (`nn.Dropout` follows eval, NGCF.py:142)."""
    if not (model.auto_train_graph and torch.is_grad_enabled() and len(u_id) > 0 and len(pos_item) > 0):
        return False
    if len(u_id) + len(pos_item) + len(neg_item) > 8192:            # beyond this GatherTriple.backward sizes its problem on the host
        return False
    if model._all_E_bytes() > min(model.auto_graph_max_bytes, 32 << 20):
        return False                                                # (32 MB: where GatherTriple.backward stays free of host syncs)
    if node_flag and model.node_dropout and model.node_dropout_mode != "device":
        return False                                                # reference-mode masks are drawn on the host: nothing to capture
    if any(p > 0 for p in model._mess_drop()) and model.mess_dropout_mode != "device":
        return False
    if not model.user_embedding.weight.requires_grad and not any(p.requires_grad for p in model._diff_params()):
        return False                                                # nothing to differentiate: the plain forward
    return not torch.cuda.is_current_stream_capturing()


def _capture_refusal(model, dev, first_stream) -> Optional[str]:
    """Why the training forward must NOT be captured right now, or None.  A captured backward that depends on anything recorded
    outside the capture ends the PROCESS on this runtime (SIGSEGV inside hipStreamEndCapture - gpurun_out/r03/gputests29b.log,
    DESIGN.md 7 - not an exception that could be caught), so everything that could smuggle such a dependency in, or run foreign
    code inside the capture, keeps the eager path."""
    for p in model._diff_params():
        if getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
            return "a differentiable parameter carries a backward / post-accumulate-grad hook"
    if model._backward_hooks or model._backward_pre_hooks:
        return "the module carries a backward hook"
    if torch.is_anomaly_enabled():
        return "autograd anomaly mode is on"
    if torch._C._autograd._top_saved_tensors_default_hooks(True) is not None:
        return "saved-tensor hooks are active"
    if torch.cuda.current_stream(dev).cuda_stream != first_stream:
        return "the current stream is not the one the first (eager) call of this shape ran on"
    return None


def forward_train_graphed(model, dev, year, u_id, age, sex, month, day, dow, pos_item, neg_item, node_flag):
    """The training forward as a hipGraph replay whose autograd node replays the captured backward (module docstring of
    `auto_train_graph`).  The first call of a shape runs eagerly (its ids are checked at once); the second captures: three
    warm-up iterations on a side stream, then the two graphs - the dropout seed state is put back afterwards, so the masks of
    the following steps are exactly those of an eager run.  Parameters are read when the graphs run: optimizer steps and
    `load_state_dict` need nothing; a replaced parameter tensor gives a new key."""
    year_idx = model._year_index(year)
    has_neg = len(neg_item) > 0
    sizes = _batch_sizes(u_id, age, sex, month, day, dow, pos_item, neg_item)
    key = _graph_key(model, dev, sizes, year_idx) + (      # + everything else a capture bakes into its kernel arguments
        bool(node_flag), model.node_dropout_mode, model.mess_dropout_mode, model.node_dropout,
        None if model.mess_dropout is None else tuple(float(x) for x in model.mess_dropout), bool(model.training))
    to_dev = lambda t: t.to(device=dev, dtype=torch.int64).contiguous()   # noqa: E731
    args = [to_dev(t) for t in (u_id, age, sex, month, day, dow, pos_item)] + ([to_dev(neg_item)] if has_neg else [])
    g = model._train_graphs.pop(key, None)
    if g is not None and not g.intact():                           # a baked buffer was replaced: these graphs are dead
        g = None
    draws = bool((node_flag and model.node_dropout) or any(p > 0 for p in model._mess_drop()))
    if draws and getattr(model, "_seed_state", None) is not None and model._seed_state_src != torch.initial_seed():
        if g is not None:
            model._train_graphs[key] = g
        return None                                                # re-seeded since the last draw: this call draws eagerly (and re-seeds in place)
    if g is not None and (g.outstanding() or _static_result_held(model, g.all_E, g._free)):
        model._train_graphs[key] = g
        return None                                                # an earlier replay still awaits its backward, or a caller kept its
                                                                   # all_*_emb (views of the graph's static all_E): this forward runs eagerly
    if g is None:
        cur = torch.cuda.current_stream(dev).cuda_stream
        if key not in model._train_seen:
            if len(model._train_seen) > 64:
                model._train_seen.clear()
            model._train_seen[key] = cur
            return None
        why = _capture_refusal(model, dev, model._train_seen[key])
        if why is not None:
            model._train_seen[key] = cur
            if not model._capture_warned:
                model._capture_warned = True
                warnings.warn(f"NGCF.auto_train_graph: the training forward is not captured ({why}); it keeps the eager path", stacklevel=3)
            return None
        for k in list(model._train_graphs)[:max(0, len(model._train_graphs) - 3)]:     # a handful of shapes (full batch, last batch)
            model._train_graphs.pop(k, None)
        # A forward that draws masks has created the seed state in its first (eager) call.  One that draws none must not create it:
        # the first drawing forward after `torch.manual_seed` uses the seeds as handed out, every later one steps them first
        # (`NGCF._device_seeds`), so a state made here would put every later mask one step ahead of the eager run's.  (When the state
        # appears later, `intact()` sees a baked pointer change and these graphs are captured once more.)
        seed_state = model._seed_state.clone() if getattr(model, "_seed_state", None) is not None else None
        model._scratch_buf(dev)
        model._status_buf(dev)
        with _eng._on(dev):                                        # (streams and graphs belong to the model's device)
            g = _TrainGraphs(model, year_idx, bool(node_flag), has_neg, args)
        if seed_state is not None:
            model._seed_state.copy_(seed_state)                    # the warm-up forwards stepped it
        if model.check_indices:
            model._raise_if_status()
    model._train_graphs[key] = g
    model._train_calls += 1
    if model.check_indices:
        model._peek_status()                                       # an earlier replay's bad id, as soon as the GPU got there
    with _eng._on(dev):
        outs = g(*args)
    if model.check_indices and model._train_calls % max(1, int(model.index_check_every)) == 0:
        model.check_indices_now()
    return outs[0], outs[1], (outs[2] if has_neg else torch.empty(0))      # (fresh tensors: `_ReplayTrain.forward` copies them out)
