"""The wrappers of the header's section "backward pass" (csrc/bwd_dense.hip, csrc/bwd_gather.hip), which `Propagate.backward`,
`GatherTriple.backward` and the multi-GPU layer pieces drive.  Like the wrappers of `layers`: no check here costs a host sync."""
from __future__ import annotations

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _row_major_ld, _stream


def bwd_pre(dN, dC, Cc, leaky, drop_p, seed, mask=None, row_ids=None):
    lib = _lib.load()
    n_rows, d = Cc.shape
    # rows padded to a multiple of 32 floats: 128-byte aligned rows at the reference's own widths too (65 -> 96), which is what
    # the fused input-gradient kernel reads dM through (16-byte pieces; columns past d are masked there)
    ldm = (d + 31) // 32 * 32
    dM = torch.empty((n_rows, ldm), dtype=torch.float32, device=Cc.device)[:, :d]
    with _on(Cc.device):
        _lib.check(lib.ngcf_layer_bwd_pre_f32(_ptr(dN), 0 if dN is None else _row_major_ld(dN, "dN"), _ptr(dC),
                                              0 if dC is None else _row_major_ld(dC, "dC"), _ptr(Cc),
                                              _row_major_ld(Cc, "C"), n_rows, d, leaky, float(drop_p), int(seed),
                                              _ptr(mask), 0 if mask is None else _row_major_ld(mask, "drop_mask"),
                                              _ptr(row_ids), _ptr(dM), ldm, _stream()))
    return dM


def bwd_weight(dM, LE, E, ws):
    """(gW1, gb1, gW2, gb2): gW1 = dM^T . (LE + E), gW2 = dM^T . (LE * E) on the fp32 matrix cores, gb2 = column sums of dM and
    gb1 = twice that (b1 enters the layer twice) from the same pass over dM (ngcf_layer_bwd_weight_f32), written straight into the
    four gradient tensors; blocks of at most 128 output rows x 128 input columns (one kernel call each)."""
    lib = _lib.load()
    n_rows, d_out = dM.shape
    d_in = int(LE.shape[1])
    gW1, gW2 = (torch.empty((d_out, d_in), dtype=torch.float32, device=dM.device) for _ in range(2))
    gb1, gb2 = (torch.empty((d_out,), dtype=torch.float32, device=dM.device) for _ in range(2))
    w = ws.get(int(lib.ngcf_bwd_weight_workspace_bytes()), dM.device)
    with _on(dM.device):
        for o0 in range(0, d_out, 128):
            o1 = min(d_out, o0 + 128)
            for c0 in range(0, d_in, 128):
                c1 = min(d_in, c0 + 128)
                a, b, c = dM[:, o0:o1], LE[:, c0:c1], E[:, c0:c1]
                _lib.check(lib.ngcf_layer_bwd_weight_f32(_ptr(a), _row_major_ld(a, "dM"), _ptr(b), _row_major_ld(b, "LE"),
                                                         _ptr(c), _row_major_ld(c, "E"), n_rows, c1 - c0, o1 - o0,
                                                         _ptr(gW1[o0:o1, c0:c1]), d_in, _ptr(gW2[o0:o1, c0:c1]), d_in,
                                                         _ptr(gb1[o0:o1]) if c0 == 0 else None, _ptr(gb2[o0:o1]) if c0 == 0 else None,
                                                         _ptr(w), w.numel(), _stream()))
    return gW1, gb1, gW2, gb2


def bwd_input(dM, w1, w2, LE, E, ws):
    """dLE, dE_direct from dM in one MFMA kernel (ngcf_layer_bwd_input_f32): dM.[W1|W2] and its combination with E / LE."""
    lib = _lib.load()
    n_rows, d_out = dM.shape
    d_in = int(LE.shape[1])
    d4 = (d_in + 31) // 32 * 32   # 128-byte aligned rows: L^T . dLE then runs on the float4 / swept kernels at any width
    dLE = torch.empty((n_rows, d4), dtype=torch.float32, device=LE.device)[:, :d_in]
    dE = torch.empty((n_rows, d4), dtype=torch.float32, device=LE.device)[:, :d_in]
    w1, w2 = w1.contiguous(), w2.contiguous()
    w = ws.get(int(lib.ngcf_layer_bwd_input_workspace_bytes(d_out)), dM.device)
    with _on(dM.device):
        _lib.check(lib.ngcf_layer_bwd_input_f32(_ptr(dM), _row_major_ld(dM, "dM"), n_rows, d_out, _ptr(w1), _ptr(w2), d_in,
                                                _ptr(LE), _row_major_ld(LE, "LE"), _ptr(E), _row_major_ld(E, "E"),
                                                _ptr(dLE), d4, _ptr(dE), d4, _ptr(w), w.numel(), _stream()))
    return dLE, dE


def add_rows(out, add):
    lib = _lib.load()
    with _on(out.device):
        _lib.check(lib.ngcf_add_rows_f32(_ptr(out), _row_major_ld(out, "out"), _ptr(add), _row_major_ld(add, "add"),
                                         out.shape[0], out.shape[1], _stream()))


def rows_sort_unique(pos, n_max):
    """`(order, rows, segptr, cnt)` of the M row ids `pos` (int64, at most `n_max`) in one launch (ngcf_rows_sort_unique): the positions
    grouped by row in batch order, the sorted distinct rows, the group bounds, their count [1] - int64 on the device, sized for M rows."""
    lib = _lib.load()
    M, dev = int(pos.numel()), pos.device
    buf = torch.empty(3 * M + 2, dtype=torch.int64, device=dev)
    order, rows, segptr, cnt = buf[:M], buf[M:2 * M], buf[2 * M:3 * M + 1], buf[3 * M + 1:]
    with _on(dev):
        _lib.check(lib.ngcf_rows_sort_unique(_ptr(pos.contiguous()), M, int(n_max), _ptr(order), _ptr(rows), _ptr(segptr), _ptr(cnt),
                                             _stream()))
    return order, rows, segptr, cnt


def segment_sum_rows(g, order, segptr, n_seg, out, rows=None, cnt=None):
    """Sums of the groups g[order[segptr[s] : segptr[s + 1]]] of rows of `g` [M, D], in a fixed order (ngcf_segment_sum_rows_f32), into
    row s of `out` [n_seg, D] - or, with `rows` and `cnt` as `rows_sort_unique` left them, the first cnt[0] into the rows rows[s] of `out`."""
    lib = _lib.load()
    D = int(g.shape[1])
    with _on(g.device):
        _lib.check(lib.ngcf_segment_sum_rows_f32(_ptr(g), D, D, _ptr(order), _ptr(segptr), int(n_seg), _ptr(rows), _ptr(cnt), _ptr(out),
                                                 D, int(out.shape[0]) if rows is not None else 0, _stream()))
