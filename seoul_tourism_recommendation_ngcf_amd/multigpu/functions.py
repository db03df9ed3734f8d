"""The exchange steps as plain calls and as autograd Functions, and the differentiable layer pieces: the TRAINING path of the
sharded engine (experiment.py:57 across ranks)."""

import ctypes as C

import torch
import torch.distributed as dist

from .. import _lib, engine as _eng
from ..all_e import _padded_rows
from .p2p import P2PCollectives


def allgather_rows(full_block: torch.Tensor, send: torch.Tensor, group=None, async_op: bool = False):
    """full_block[W*m, d] <- every rank's send[m, d], rank-major (one collective, no unpack)."""
    assert full_block.is_contiguous() and send.is_contiguous()
    assert full_block.shape[0] == send.shape[0] * dist.get_world_size(group)
    return dist.all_gather_into_tensor(full_block, send, group=group, async_op=async_op)


def owner_rows_sum(local_rows: torch.Tensor, owned: torch.Tensor, group=None) -> torch.Tensor:
    """Rows served by their owning rank (others contribute zeros), summed over ranks: every rank ends up with
    all B rows.  x + 0 is exact, so values are the owners' bits."""
    out = torch.where(owned[:, None], local_rows, torch.zeros((), dtype=local_rows.dtype, device=local_rows.device))
    dist.all_reduce(out, group=group)
    return out


class _CabiAllGather:
    """`ngcf_allgather_rows` (include/ngcf_hip.h): ncclAllGather on a communicator handle, issued by the library on a
    stream of its own.  Opt-in (NGCF_DIST_COLLECTIVES=cabi, backend "nccl" only): the handle is the process group's own
    RCCL communicator.  The default path is `torch.distributed`'s all_gather_into_tensor, which does the same thing."""

    def __init__(self, group, device):
        pg = group if group is not None else dist.group.WORLD
        backend = pg._get_backend(torch.device(device))
        dist.barrier(group=group)                                  # the communicator exists after the first collective
        self.comm = C.c_void_p(int(backend._comm_ptr()))
        self.stream = torch.cuda.Stream(device=device)

    def __call__(self, full_block: torch.Tensor, send: torch.Tensor):
        cur = torch.cuda.current_stream(send.device)
        self.stream.wait_stream(cur)                               # the rows were produced on the compute stream
        _lib.check(_lib.load().ngcf_allgather_rows(self.comm, C.c_void_p(send.data_ptr()), C.c_void_p(full_block.data_ptr()),
                                                   send.shape[0], send.shape[1], C.c_void_p(self.stream.cuda_stream)))
        send.record_stream(self.stream)
        full_block.record_stream(self.stream)
        return self

    def wait(self):
        torch.cuda.current_stream().wait_stream(self.stream)


def _reduce_scatter_rows(full: torch.Tensor, group) -> torch.Tensor:
    """own[m, d] = sum over ranks of full[rank*m:(rank+1)*m] (gloo has no reduce-scatter: all-reduce + own rows)."""
    if isinstance(group, P2PCollectives):
        return group.reduce_scatter(full)
    W, r = dist.get_world_size(group), dist.get_rank(group)
    m = full.shape[0] // W
    if dist.get_backend(group) == "nccl":
        out = torch.empty((m, full.shape[1]), dtype=full.dtype, device=full.device)
        dist.reduce_scatter_tensor(out, full.contiguous(), group=group)
        return out
    tmp = full.contiguous().clone()
    dist.all_reduce(tmp, group=group)
    return tmp[r * m:(r + 1) * m].clone()


def _all_gather_rows(send: torch.Tensor, comm) -> torch.Tensor:
    """`comm`: a process group (or None = the default group) for torch.distributed, or a `P2PCollectives` for the CU-free exchange."""
    if isinstance(comm, P2PCollectives):
        return comm.all_gather(send)
    full = torch.empty((send.shape[0] * dist.get_world_size(comm), send.shape[1]), dtype=send.dtype, device=send.device)
    dist.all_gather_into_tensor(full, send.contiguous(), group=comm)
    return full


class AllGatherRows(torch.autograd.Function):
    """full[W*m, d] = every rank's send[m, d], rank-major.  Adjoint: reduce-scatter of the gradient (every rank used every row)."""

    @staticmethod
    def forward(ctx, send, comm):
        ctx.comm = comm
        return _all_gather_rows(send, comm)

    @staticmethod
    def backward(ctx, g):
        return _reduce_scatter_rows(g, ctx.comm), None


class ReduceScatterRows(torch.autograd.Function):
    """own[m, d] = sum over ranks of their full[rank*m:(rank+1)*m].  Adjoint: all-gather of the gradient."""

    @staticmethod
    def forward(ctx, full, comm):
        ctx.comm = comm
        return _reduce_scatter_rows(full, comm)

    @staticmethod
    def backward(ctx, g):
        return _all_gather_rows(g, ctx.comm), None


class OwnerRowsSum(torch.autograd.Function):
    """`owner_rows_sum` with its adjoint.  Every rank computes the SAME loss from the same gathered rows, so the gradient of a
    served row is that loss's gradient on the rank that served it and nothing elsewhere - no exchange in the backward."""

    @staticmethod
    def forward(ctx, local_rows, owned, group):
        ctx.save_for_backward(owned)
        return owner_rows_sum(local_rows, owned, group)

    @staticmethod
    def backward(ctx, g):
        (owned,) = ctx.saved_tensors
        return torch.where(owned[:, None], g, torch.zeros((), dtype=g.dtype, device=g.device)), None, None


class SpmmFn(torch.autograd.Function):
    """LE = A . E on the HIP SpMM with A^T given as a second CSR: the backward is the product with that one."""

    @staticmethod
    def forward(ctx, E, csr, csr_t, ws):
        ctx.csr_t, ctx.ws = csr_t, ws
        return _eng.spmm(csr, E.detach(), ws=ws)

    @staticmethod
    def backward(ctx, g):
        gp = _padded_rows(g.shape[0], g.shape[1], g.device)
        gp.copy_(g)                                                # 128-byte aligned rows for the gather
        return _eng.spmm(ctx.csr_t, gp, ws=ctx.ws), None, None, None


class DenseLayerFn(torch.autograd.Function):
    """(carry, norm) of one layer's dense half (NGCF.py:131-146, eval-mode: no message dropout) for a slab of rows, with the
    hand-written backward kernels of engine.backward (normalise / LeakyReLU backward, MFMA weight and input gradients)."""

    @staticmethod
    def forward(ctx, LE, E, W1, b1, W2, b2, ws):
        n, d_out = LE.shape[0], W1.shape[0]
        carry = _padded_rows(n, d_out, LE.device)
        norm = torch.empty((n, d_out), dtype=torch.float32, device=LE.device)
        if n:
            _eng.layer_dense(LE.detach(), E.detach(), W1.detach(), b1.detach(), W2.detach(), b2.detach(), carry, norm, ws)
        ctx.ws = ws
        ctx.save_for_backward(LE.detach(), E.detach(), carry, W1.detach(), W2.detach())
        return carry, norm

    @staticmethod
    def backward(ctx, dC, dN):
        LE, E, carry, W1, W2 = ctx.saved_tensors
        n, d_in = LE.shape
        if n == 0:
            z = torch.zeros_like
            return z(LE), z(E), z(W1), W1.new_zeros(W1.shape[0]), z(W2), W2.new_zeros(W2.shape[0]), None
        dM = _eng.backward.bwd_pre(dN.contiguous() if dN is not None else None, dC.contiguous() if dC is not None else None, carry,
                         _eng.LEAKY_SLOPE, 0.0, 0)
        gW1, gb1, gW2, gb2 = _eng.backward.bwd_weight(dM, LE, E, ctx.ws)
        dLE, dE = _eng.backward.bwd_input(dM, W1, W2, LE, E, ctx.ws)
        return dLE, dE, gW1, gb1, gW2, gb2, None


class _SumGrads(torch.autograd.Function):
    """Identity on the (replicated) parameters; its backward makes every parameter's gradient complete on every rank - once per
    parameter and step, as in data-parallel training.

    `slabs` = {position in `params`: row bounds per rank}: that parameter (the user table) is read by rank r through rows
    [bounds[r], bounds[r+1]) only, so its gradient is non-zero in that slab only and the slabs are disjoint: an ALL-GATHER of the
    slabs (padded to the largest) gives every rank the full gradient - (W-1)/W x |table| received per rank instead of the
    2 (W-1)/W x |table| of a ring all-reduce of W dense [U, d0] matrices that are zero outside one slab each (r04; at C3 / W = 8:
    448 MB instead of 896 MB per rank and step for the 512 MB user table).  Everything else (the item table - every rank's user rows
    gather from all items -, the weights) is summed by an all-reduce."""

    @staticmethod
    def forward(ctx, group, slabs, *params):
        ctx.group, ctx.slabs = group, dict(slabs or {})
        return tuple(p.view_as(p) for p in params)

    @staticmethod
    def backward(ctx, *grads):
        out = []
        W = dist.get_world_size(ctx.group)
        r = dist.get_rank(ctx.group)
        for i, gr in enumerate(grads):
            if gr is None:
                out.append(None)
                continue
            gr = gr.contiguous()
            bounds = ctx.slabs.get(i)
            if bounds is None or W == 1:
                dist.all_reduce(gr, group=ctx.group)
                out.append(gr)
                continue
            mx = max(max(bounds[q + 1] - bounds[q] for q in range(W)), 1)
            send = gr.new_zeros((mx,) + tuple(gr.shape[1:]))
            send[:bounds[r + 1] - bounds[r]] = gr[bounds[r]:bounds[r + 1]]
            full = gr.new_empty((W * mx,) + tuple(gr.shape[1:]))
            dist.all_gather_into_tensor(full, send, group=ctx.group)
            res = torch.zeros_like(gr)                             # (rows no rank reads keep a zero gradient)
            for q in range(W):
                n_q = bounds[q + 1] - bounds[q]
                if n_q:
                    res[bounds[q]:bounds[q + 1]] = full[q * mx:q * mx + n_q]
            out.append(res)
        return (None, None, *out)
