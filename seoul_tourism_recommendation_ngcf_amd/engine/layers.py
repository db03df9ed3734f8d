"""The wrappers of the training step's hot path, a dozen calls per step: the header's sections "propagation" (csrc/spmm*.hip,
csrc/dense*.hip), "feature injection", "gathers" and "BPR" (csrc/ops.hip).  They stay short: no check here may cost a host sync or
more than a few comparisons (see `_on` and `_stream`)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib
from ._plumbing import Workspace, _f32c, _on, _ptr, _row_major_ld, _seed_array, _stream
from .csr import LaplacianCSR

LEAKY_SLOPE = 0.2            # NGCF.py:140


def spmm(csr: LaplacianCSR, E: torch.Tensor, out: Optional[torch.Tensor] = None, ws: Optional[Workspace] = None,
         edge_drop=None):
    """LE = L.E (NGCF.py:130) through ngcf_spmm_csr_f32.

    `edge_drop = (seeds, p, transposed)` applies device-side node dropout (ngcf_spmm_csr_dropout_f32): `seeds` the
    cumulative list of 64-bit layer seeds, `p` the drop probability, `transposed` true when `csr` holds L^T (the mask is
    keyed by an entry's row and column in L, so L^T loses the entries L lost)."""
    lib = _lib.load()
    _f32c(E, "E")
    d = int(E.shape[1])
    if E.shape[0] != csr.n_cols:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({csr.n_rows}x{csr.n_cols} and {tuple(E.shape)})")
    d_view = d
    if out is None:     # rows padded to a multiple of 32 floats (128-byte aligned rows: the float4 / swept kernels apply at any d)
        out = torch.empty((csr.n_rows, (d + 31) // 32 * 32), dtype=torch.float32, device=E.device)[:, :d]
        # the rule of ngcf_layer_fused_f32 (csrc/dense.hip), so that both forward paths produce the same bits: a width that is
        # not a multiple of 4 on a small (launch-bound) matrix is multiplied up to the next multiple of 4 when the gathered rows
        # are 16-byte aligned and padded - the extra columns land in the padding of `out`
        d = int(lib.ngcf_spmm_product_width(csr._h, _ptr(E), _row_major_ld(E, "E"), d))
    ws = ws or Workspace()
    nb = csr.spmm_workspace_bytes(d)
    w = ws.get(nb, E.device)
    with _on(E.device):
        if edge_drop is None:
            _lib.check(lib.ngcf_spmm_csr_f32(csr._h, _ptr(E), _row_major_ld(E, "E"), d, _ptr(out),
                                             _row_major_ld(out, "out"), _ptr(w), w.numel(), _stream()))
        else:
            seeds, p, transposed = edge_drop
            _lib.check(lib.ngcf_spmm_csr_dropout_f32(csr._h, _ptr(E), _row_major_ld(E, "E"), d, _ptr(out), _row_major_ld(out, "out"),
                                                     float(p), _seed_array(seeds), len(seeds), 1 if transposed else 0,
                                                     _ptr(w), w.numel(), _stream()))
    assert out.shape[1] == d_view
    return out


def spmm_t_rows(csr_t: LaplacianCSR, slot: torch.Tensor, X: torch.Tensor, init: Optional[torch.Tensor], out: torch.Tensor,
                ws: Workspace, edge_drop=None):
    """out = init + L^T . X for a row-sparse X given compacted (ngcf_spmm_t_rows_f32): `slot` int32[N] maps a matrix row to its
    row of X / init or -1; every row of `out` is written, every sum runs in a fixed order (no atomics).  `edge_drop = (seeds, p)`:
    device-side node dropout of the forward product."""
    lib = _lib.load()
    _f32c(X, "X"), _f32c(out, "out")
    if slot.dtype != torch.int32 or slot.numel() != csr_t.n_cols or out.shape[0] != csr_t.n_rows or X.shape[1] != out.shape[1]:
        raise RuntimeError("spmm_t_rows: shape mismatch")
    if init is not None and tuple(init.shape) != tuple(X.shape):
        raise RuntimeError("spmm_t_rows: init must have the shape of X")
    seeds, p = edge_drop if edge_drop is not None else ((), 0.0)
    d = int(X.shape[1])
    w = ws.get(csr_t.spmm_workspace_bytes(min(d, 512)), X.device)
    with _on(X.device):
        _lib.check(lib.ngcf_spmm_t_rows_f32(csr_t._h, _ptr(slot), _ptr(X), _row_major_ld(X, "X"), d, _ptr(init),
                                            0 if init is None else _row_major_ld(init, "init"), _ptr(out), _row_major_ld(out, "out"),
                                            float(p), _seed_array(seeds), len(seeds), _ptr(w), w.numel(), _stream()))


def spmm_t_rows_path(csr_t: LaplacianCSR, d: int, ws: Workspace, device) -> str:
    """'bitmap' or 'slot': the kernel `spmm_t_rows` would run on `csr_t` at width d with the scratch `ws` on `device` under the
    current options (ngcf_spmm_t_rows_path: host code, nothing is launched; for tests and tools).  The workspace size asked about
    is the one `spmm_t_rows` passes: that of `ws` once it holds ngcf_spmm_workspace_bytes(csr_t, min(d, 512)) bytes."""
    lib = _lib.load()
    w = ws.get(csr_t.spmm_workspace_bytes(min(int(d), 512)), device)
    name = lib.ngcf_spmm_t_rows_path(csr_t._h, int(d), w.numel())
    if name is None:
        raise RuntimeError(_lib.last_error())
    return name.decode()


def layer_fused(csr: LaplacianCSR, E_gather: torch.Tensor, E_self: torch.Tensor, W1, b1, W2, b2,
                carry: Optional[torch.Tensor], norm: torch.Tensor, ws: Workspace,
                drop_p: float = 0.0, drop_seed: int = 0, drop_mask: Optional[torch.Tensor] = None):
    """One propagation layer (NGCF.py:130-146) through ngcf_layer_fused_f32.  `drop_mask` [n_rows, d_out]: the noise
    tensor of nn.Dropout (0 or 1/(1-p)) drawn by the caller; None with drop_p > 0: the in-kernel hash stream."""
    lib = _lib.load()
    d_in, d_out = int(W1.shape[1]), int(W1.shape[0])
    for t, nm in ((E_gather, "E_gather"), (E_self, "E_self"), (W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2"), (norm, "norm")):
        _f32c(t, nm)
    if E_gather.shape[1] != d_in or E_self.shape[1] != d_in:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(E_self.shape)} and {d_in}x{d_out})")
    if E_gather.shape[0] != csr.n_cols or E_self.shape[0] != csr.n_rows or norm.shape[0] != csr.n_rows:
        raise RuntimeError("layer_fused: row counts do not match the Laplacian")
    W1, W2, b1, b2 = W1.contiguous(), W2.contiguous(), b1.contiguous(), b2.contiguous()
    nb = csr.layer_workspace_bytes(d_in, d_out)
    w = ws.get(nb, norm.device)
    with _on(norm.device):
        _lib.check(lib.ngcf_layer_fused_f32(
            csr._h, _ptr(E_gather), _row_major_ld(E_gather, "E_gather"), _ptr(E_self), _row_major_ld(E_self, "E_self"),
            d_in, _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), d_out, LEAKY_SLOPE, float(drop_p), int(drop_seed),
            _ptr(drop_mask), 0 if drop_mask is None else _row_major_ld(drop_mask, "drop_mask"),
            _ptr(carry), 0 if carry is None else _row_major_ld(carry, "carry"),
            _ptr(norm), _row_major_ld(norm, "norm"), _ptr(w), w.numel(), _stream()))


def layer_dense(LE: torch.Tensor, E_self: torch.Tensor, W1, b1, W2, b2, carry, norm, ws: Workspace,
                drop_p: float = 0.0, drop_seed: int = 0, drop_mask: Optional[torch.Tensor] = None):
    """Dense half of a layer (NGCF.py:131-146) on an existing LE, through ngcf_layer_dense_f32."""
    lib = _lib.load()
    d_in, d_out = int(W1.shape[1]), int(W1.shape[0])
    W1, W2, b1, b2 = W1.contiguous(), W2.contiguous(), b1.contiguous(), b2.contiguous()
    nb = int(lib.ngcf_dense_workspace_bytes(d_in, d_out))
    if nb < 0:
        raise RuntimeError(f"unsupported layer widths d_in={d_in} d_out={d_out}")
    w = ws.get(nb, norm.device)
    with _on(norm.device):
        _lib.check(lib.ngcf_layer_dense_f32(
            _ptr(LE), _row_major_ld(LE, "LE"), _ptr(E_self), _row_major_ld(E_self, "E_self"), LE.shape[0], d_in,
            _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), d_out, LEAKY_SLOPE, float(drop_p), int(drop_seed),
            _ptr(drop_mask), 0 if drop_mask is None else _row_major_ld(drop_mask, "drop_mask"),
            _ptr(carry), 0 if carry is None else _row_major_ld(carry, "carry"),
            _ptr(norm), _row_major_ld(norm, "norm"), _ptr(w), w.numel(), _stream()))


def copy_rows(src: torch.Tensor, dst: torch.Tensor, dst2: Optional[torch.Tensor] = None):
    """dst[:, :] = src (strided row copy, ngcf_copy_rows_f32); with `dst2` also dst2[:, :] = src in the same pass."""
    lib = _lib.load()
    _f32c(src, "src"), _f32c(dst, "dst")
    if src.shape != dst.shape or (dst2 is not None and dst2.shape != src.shape):
        raise RuntimeError(f"copy_rows: shape mismatch {tuple(src.shape)} vs {tuple(dst.shape)}")
    if src.shape[0] == 0:
        return
    with _on(dst.device):
        if dst2 is None:
            _lib.check(lib.ngcf_copy_rows_f32(_ptr(src), _row_major_ld(src, "src"), _ptr(dst), _row_major_ld(dst, "dst"),
                                              src.shape[0], src.shape[1], _stream()))
        else:
            _lib.check(lib.ngcf_copy_rows2_f32(_ptr(src), _row_major_ld(src, "src"), _ptr(dst), _row_major_ld(dst, "dst"),
                                               _ptr(_f32c(dst2, "dst2")), _row_major_ld(dst2, "dst2"), src.shape[0],
                                               src.shape[1], _stream()))


def copy_rows_indexed(src: torch.Tensor, dst: torch.Tensor, idx: torch.Tensor):
    """dst[idx[b], :] = src[idx[b], :] (ngcf_copy_rows_indexed_f32): the rows a batch touched, ids out of range skipped."""
    lib = _lib.load()
    _f32c(src, "src"), _f32c(dst, "dst")
    if src.shape != dst.shape or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.device != dst.device:
        raise RuntimeError("copy_rows_indexed: src and dst must have one shape, idx must be a contiguous int64 tensor on their device")
    if idx.numel() == 0 or src.shape[0] == 0:
        return
    with _on(dst.device):
        _lib.check(lib.ngcf_copy_rows_indexed_f32(_ptr(src), _row_major_ld(src, "src"), _ptr(dst), _row_major_ld(dst, "dst"), _ptr(idx),
                                                  idx.numel(), src.shape[0], src.shape[1], _stream()))


def gather_rows(table: torch.Tensor, idx: torch.Tensor, status: torch.Tensor, row_off: int = 0,
                n_idx_rows: Optional[int] = None) -> torch.Tensor:
    """out[b] = table[row_off + idx[b]] (NGCF.py:151-155), bit-exact copies; fresh output tensor."""
    lib = _lib.load()
    _f32c(table, "table")
    idx = idx.to(device=table.device, dtype=torch.int64).contiguous()
    d = int(table.shape[1])
    B = int(idx.numel())
    out = torch.empty((B, d), dtype=torch.float32, device=table.device)
    if n_idx_rows is None:
        n_idx_rows = int(table.shape[0]) - row_off
    with _on(table.device):
        _lib.check(lib.ngcf_gather_rows_f32(_ptr(table), _row_major_ld(table, "table"), d, _ptr(idx), B, row_off,
                                            n_idx_rows, _ptr(out), d, _ptr(status), _stream()))
    return out


def gather_rows3(table: torch.Tensor, sets, status: torch.Tensor):
    """The (users, positive items, negative items) gathers of NGCF.py:151-155 in one launch.  `sets` = three
    `(idx or None, row_off, n_idx_rows)`; returns three fresh tensors (`None` where idx is None).  Bit-exact copies."""
    lib = _lib.load()
    _f32c(table, "table")
    d = int(table.shape[1])
    args, outs = [], []
    for idx, row_off, n_rows in sets:
        if idx is None:
            args += [None, 0, 0, 0, None]
            outs.append(None)
            continue
        idx = idx.to(device=table.device, dtype=torch.int64).contiguous()
        out = torch.empty((int(idx.numel()), d), dtype=torch.float32, device=table.device)
        args += [_ptr(idx), int(idx.numel()), int(row_off), int(n_rows), _ptr(out)]
        outs.append(out)
    with _on(table.device):
        _lib.check(lib.ngcf_gather_rows3_f32(_ptr(table), _row_major_ld(table, "table"), d, *args, d, _ptr(status), _stream()))
    return outs


def feature_inject(user_w: torch.Tensor, tables: Sequence[torch.Tensor], idx: Sequence[torch.Tensor],
                   u_id: torch.Tensor, emb_ratio: float, scratch: torch.Tensor, status: torch.Tensor):
    """user_w[u_id] = user_w[u_id]*(1-r) + cat(feature rows)*r in place (NGCF.py:103-115)."""
    lib = _lib.load()
    _f32c(user_w, "user_embedding.weight")
    if not user_w.is_contiguous():
        raise RuntimeError("user_embedding.weight must be contiguous")
    dev = user_w.device
    tabs = [_f32c(t, "feature table").contiguous() for t in tables]
    ids = [i.to(device=dev, dtype=torch.int64).contiguous() for i in idx]
    u_id = u_id.to(device=dev, dtype=torch.int64).contiguous()
    B = int(u_id.numel())
    for i in ids:
        if int(i.numel()) != B:
            raise RuntimeError("shape mismatch: feature index vectors and u_id differ in length")
    fw = int(tabs[0].shape[1])
    t_arr = (C.c_void_p * 5)(*[t.data_ptr() for t in tabs])
    i_arr = (C.c_void_p * 5)(*[i.data_ptr() for i in ids])
    c_arr = (C.c_int64 * 5)(*[int(t.shape[0]) for t in tabs])
    with _on(dev):
        _lib.check(lib.ngcf_feature_inject_f32(_ptr(user_w), user_w.shape[1], user_w.shape[0], user_w.shape[1],
                                               t_arr, i_arr, c_arr, fw, _ptr(u_id), B, float(emb_ratio),
                                               _ptr(scratch), _ptr(status), _stream()))
    return ids  # keep the converted index tensors alive until the stream has consumed them


def bpr_loss(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, weight_decay: float, batch_size: float,
             ws: Workspace) -> torch.Tensor:
    """Fused BPR (bprloss.py:15-22) through ngcf_bpr_fused_f32 -> 0-dim device tensor."""
    lib = _lib.load()
    for t, nm in ((u, "u"), (p, "pos"), (n, "neg")):
        _f32c(t, nm)
        if t.dim() != 2:
            raise RuntimeError(f"BPR: {nm} must be 2-D, got shape {tuple(t.shape)}")
    D = int(u.shape[1])
    if p.shape[1] != D or n.shape[1] != D:
        raise RuntimeError(f"The size of tensor a ({D}) must match the size of tensor b ({p.shape[1]}/{n.shape[1]}) "
                           "at non-singleton dimension 1")
    u, p, n = u.contiguous(), p.contiguous(), n.contiguous()
    R = max(u.shape[0], p.shape[0], n.shape[0])
    nb = int(lib.ngcf_bpr_workspace_bytes(R))
    w = ws.get(nb, u.device)
    loss = torch.empty((), dtype=torch.float32, device=u.device)
    with _on(u.device):
        _lib.check(lib.ngcf_bpr_fused_f32(_ptr(u), u.shape[0], _ptr(p), p.shape[0], _ptr(n), n.shape[0], D,
                                          float(weight_decay), float(batch_size), _ptr(loss), _ptr(w), w.numel(),
                                          _stream()))
    return loss


def bpr_backward(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, weight_decay: float, batch_size: float, grad_out: torch.Tensor):
    """(du, dp, dn) of `bpr_loss` times the upstream scalar `grad_out`, through ngcf_bpr_backward_f32."""
    lib = _lib.load()
    u, p, n = u.contiguous(), p.contiguous(), n.contiguous()
    du, dp, dn = torch.empty_like(u), torch.empty_like(p), torch.empty_like(n)
    g = grad_out.to(torch.float32).contiguous()
    with _on(u.device):
        _lib.check(lib.ngcf_bpr_backward_f32(_ptr(u), u.shape[0], _ptr(p), p.shape[0], _ptr(n), n.shape[0], u.shape[1],
                                             float(weight_decay), float(batch_size), _ptr(g), _ptr(du), _ptr(dp), _ptr(dn), _stream()))
    return du, dp, dn
