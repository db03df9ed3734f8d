"""Host side of the propagation engine: thin, typed wrappers over the C ABI (include/ngcf_hip.h).

Everything here hands `tensor.data_ptr()` + the current HIP stream to libngcf_hip.so.  torch is
used for device memory and streams only; no tensor arithmetic of the hot path happens in torch.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

LEAKY_SLOPE = 0.2            # NGCF.py:140


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


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL = _NullCtx()


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


class LaplacianCSR:
    """Device CSR of one Laplacian slice (or a row slab of it), built from the COO of `lap_list[k]`.

    Replaces `self.lap_list[year_idx].to(self.device)` + the COO SpMM set-up of NGCF.py:118,130.
    """

    def __init__(self, handle: int, keep_alive=()):
        self._h = C.c_void_p(handle)
        self._keep = keep_alive
        lib = _lib.load()
        self.n_rows = int(lib.ngcf_csr_n_rows(self._h))
        self.n_cols = int(lib.ngcf_csr_n_cols(self._h))
        self.nnz = int(lib.ngcf_csr_nnz(self._h))

    @property
    def max_row_len(self) -> int:
        """Stored entries of the longest row."""
        return int(_lib.load().ngcf_csr_max_row_len(self._h))

    # -- constructors ---------------------------------------------------------------------
    @classmethod
    def from_coo(cls, rows: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor, n_rows: int, n_cols: int):
        lib = _lib.load()
        for t, nm in ((rows, "rows"), (cols, "cols"), (vals, "vals")):
            _require_device(t, "Laplacian " + nm)
        rows = rows.contiguous().to(torch.int64)
        cols = cols.contiguous().to(torch.int64)
        vals = vals.contiguous().to(torch.float32)
        if not (rows.numel() == cols.numel() == vals.numel()):
            raise RuntimeError("Laplacian COO arrays differ in length")
        out = C.c_void_p()
        with _on(vals.device):
            _lib.check(lib.ngcf_csr_from_coo(_ptr(rows), _ptr(cols), _ptr(vals), rows.numel(), n_rows, n_cols,
                                             C.byref(out), _stream()))
        return cls(out.value)

    @classmethod
    def from_sparse_coo(cls, L: torch.Tensor, device, row_range=None):
        """From a torch sparse COO tensor (the element type of `lap_list`, matrix.py:79-83)."""
        if not L.is_sparse:
            raise RuntimeError("lap_list entries must be torch sparse COO tensors (matrix.py:79-83)")
        idx = L._indices().to(device)
        val = L._values().to(device=device, dtype=torch.float32)
        n_rows, n_cols = int(L.shape[0]), int(L.shape[1])
        rows, cols = idx[0], idx[1]
        if row_range is not None:
            lo, hi = row_range
            sel = (rows >= lo) & (rows < hi)
            rows, cols, val = rows[sel] - lo, cols[sel], val[sel]
            n_rows = hi - lo
        return cls.from_coo(rows, cols, val, n_rows, n_cols)

    @classmethod
    def from_csr_arrays(cls, rowptr: torch.Tensor, colidx: torch.Tensor, vals: torch.Tensor, n_cols: int):
        lib = _lib.load()
        for t, nm in ((rowptr, "rowptr"), (colidx, "colidx"), (vals, "vals")):
            _require_device(t, "CSR " + nm)
        assert rowptr.dtype == torch.int64 and colidx.dtype == torch.int32 and vals.dtype == torch.float32
        rowptr, colidx, vals = rowptr.contiguous(), colidx.contiguous(), vals.contiguous()
        out = C.c_void_p()
        with _on(vals.device):
            _lib.check(lib.ngcf_csr_from_arrays(_ptr(rowptr), _ptr(colidx), _ptr(vals), rowptr.numel() - 1, n_cols,
                                                colidx.numel(), C.byref(out), _stream()))
        return cls(out.value, keep_alive=(rowptr, colidx, vals))

    def filtered(self, keep: torch.Tensor, entry_map: Optional[torch.Tensor] = None, nnz_kept: int = -1,
                 reuse: Optional["LaplacianCSR"] = None) -> "LaplacianCSR":
        """Thinned copy on the device (ngcf_csr_filter): the entries e with keep[entry_map[e]] (entry_map None: keep[e]) in this
        matrix's order - the reference's `sparse_dropout` (NGCF.py:93-100) without a COO rebuild, a host round trip or, when
        `reuse` (the object a previous call returned for the same source shape) is given, an allocation.  `keep`: device uint8 /
        bool; `entry_map`: device int32.  The copy borrows this object's segment lists and keeps it alive."""
        lib = _lib.load()
        _require_device(keep, "keep flags")
        if keep.dtype not in (torch.uint8, torch.bool) or not keep.is_contiguous():
            raise RuntimeError("filtered: keep must be a contiguous uint8 / bool tensor")
        if entry_map is not None and (entry_map.dtype != torch.int32 or not entry_map.is_contiguous() or entry_map.numel() != self.nnz):
            raise RuntimeError("filtered: entry_map must be a contiguous int32 tensor with one element per stored entry")
        if entry_map is None and keep.numel() != self.nnz:
            raise RuntimeError(f"filtered: {keep.numel()} keep flags for {self.nnz} stored entries")
        out = C.c_void_p(reuse._h.value if reuse is not None and reuse._h.value else None)
        with _on(keep.device):
            rc = lib.ngcf_csr_filter(self._h, _ptr(keep), _ptr(entry_map), int(nnz_kept), C.byref(out), _stream())
        if reuse is not None:                              # the handle moved into the returned object (or was replaced by the library)
            reuse._h = C.c_void_p(0 if rc == _lib.OK else (out.value or 0))
        _lib.check(rc)
        res = LaplacianCSR(out.value, keep_alive=(self,))
        res.src_nnz = self.nnz
        return res

    @property
    def filter_pos(self) -> int:
        """Device address of the int32[source nnz + 1] scan `pos` of a filtered copy (position of every kept entry)."""
        return int(_lib.load().ngcf_csr_filter_pos(self._h) or 0)

    # -- misc -----------------------------------------------------------------------------
    def plan(self, seg_len: int):
        _lib.check(_lib.load().ngcf_csr_plan(self._h, int(seg_len), _stream()))

    def set_mode(self, mode: int):
        """0 row-wise kernels (d-sliced where it pays), 1 row-wise without slicing, 2 L2-swept kernel wherever the shape
        allows (tests), 3 L2-swept kernel on the row groups where it is expected to pay (long-lived matrices)."""
        _lib.check(_lib.load().ngcf_csr_set_mode(self._h, int(mode), _stream()))

    @property
    def n_segments(self) -> int:
        return int(_lib.load().ngcf_csr_n_segments(self._h))

    @property
    def swept_rows(self) -> int:
        """Rows covered by L2-swept parts (0: all products of this CSR use the row-wise kernels)."""
        return int(_lib.load().ngcf_csr_swept_rows(self._h))

    def layer_workspace_bytes(self, d_in: int, d_out: int) -> int:
        n = int(_lib.load().ngcf_layer_workspace_bytes(self._h, d_in, d_out))
        if n < 0:
            raise RuntimeError(f"unsupported layer widths d_in={d_in} d_out={d_out} (1..512)")
        return n

    def spmm_workspace_bytes(self, d: int) -> int:
        return int(_lib.load().ngcf_spmm_workspace_bytes(self._h, d))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().ngcf_csr_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class Workspace:
    """A grow-only byte buffer on one device, handed to the kernels as scratch."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf


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
            arr = (C.c_uint64 * max(len(seeds), 1))(*[int(x) & (2 ** 64 - 1) for x in seeds])
            _lib.check(lib.ngcf_spmm_csr_dropout_f32(csr._h, _ptr(E), _row_major_ld(E, "E"), d, _ptr(out),
                                                     _row_major_ld(out, "out"), float(p), arr, len(seeds), 1 if transposed else 0,
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
    arr = (C.c_uint64 * max(len(seeds), 1))(*[int(x) & (2 ** 64 - 1) for x in seeds])
    d = int(X.shape[1])
    w = ws.get(csr_t.spmm_workspace_bytes(min(d, 512)), X.device)
    with _on(X.device):
        _lib.check(lib.ngcf_spmm_t_rows_f32(csr_t._h, _ptr(slot), _ptr(X), _row_major_ld(X, "X"), d, _ptr(init),
                                            0 if init is None else _row_major_ld(init, "init"), _ptr(out), _row_major_ld(out, "out"),
                                            float(p), arr, len(seeds), _ptr(w), w.numel(), _stream()))


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


def topk_rows(scores: torch.Tensor, k: int):
    """`torch.topk(scores, k)` for a 2-D fp32 score matrix (values, int64 indices), through ngcf_topk_rows_f32."""
    lib = _lib.load()
    _f32c(scores, "scores")
    if scores.dim() != 2:
        raise RuntimeError("topk_rows: expected a 2-D score matrix")
    n_rows, n_cols = int(scores.shape[0]), int(scores.shape[1])
    scores = scores if scores.stride(1) == 1 else scores.contiguous()
    vals = torch.empty((n_rows, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((n_rows, k), dtype=torch.int64, device=scores.device)
    with _on(scores.device):
        _lib.check(lib.ngcf_topk_rows_f32(_ptr(scores), _row_major_ld(scores, "scores"), n_rows, n_cols, int(k), _ptr(vals),
                                          _ptr(idx), _stream()))
    return vals, idx


def recommend_topk(u_emb: torch.Tensor, item_emb: torch.Tensor, k: int, return_scores: bool = False):
    """Scores of every item for every user row and their top-k (experiment.py:93,104-111; demo.py:233-235) in ONE launch of a
    hand-written kernel (ngcf_recommend_topk_f32): score tiles through LDS, then radix select + bitonic sort per row.
    Returns (values [B, k], int64 indices [B, k]); with `return_scores` also the [B, n_items] score matrix (what
    `torch.mm(u_emb, item_emb.T)` is in the reference)."""
    lib = _lib.load()
    _f32c(u_emb, "u_emb"), _f32c(item_emb, "item_emb")
    if u_emb.dim() != 2 or item_emb.dim() != 2 or u_emb.shape[1] != item_emb.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(u_emb.shape)} and {tuple(item_emb.t().shape)})")
    B, D, n_items = int(u_emb.shape[0]), int(u_emb.shape[1]), int(item_emb.shape[0])
    u_emb = u_emb if u_emb.stride(1) == 1 else u_emb.contiguous()
    item_emb = item_emb if item_emb.stride(1) == 1 else item_emb.contiguous()
    scores = torch.empty((B, n_items), dtype=torch.float32, device=u_emb.device)
    vals = torch.empty((B, k), dtype=torch.float32, device=u_emb.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=u_emb.device)
    with _on(u_emb.device):
        _lib.check(lib.ngcf_recommend_topk_f32(_ptr(u_emb), _row_major_ld(u_emb, "u_emb"), B, _ptr(item_emb),
                                               _row_major_ld(item_emb, "item_emb"), n_items, D, int(k), _ptr(scores), n_items,
                                               _ptr(vals), _ptr(idx), _stream()))
    return (vals, idx, scores) if return_scores else (vals, idx)


def shard_plan(rowptr_host: torch.Tensor, row_begin: int, row_end: int, world: int):
    """nnz-balanced contiguous cut of rows [row_begin,row_end) into `world` ranges (host helper)."""
    lib = _lib.load()
    rp = rowptr_host.to(device="cpu", dtype=torch.int64).contiguous()
    bounds = (C.c_int64 * (world + 1))()
    _lib.check(lib.ngcf_shard_plan(C.cast(rp.data_ptr(), C.POINTER(C.c_int64)), row_begin, row_end, world, bounds))
    return [int(b) for b in bounds]


# ---- full-catalogue ranking and held-out metrics (ngcf_rank_topk_f32 / ngcf_rank_metrics, csrc/rank.hip) --------------------------
RANK_K_MAX = 256


class ItemSets:
    """A sorted item list per user in CSR form - the exclusion set (train items) or the truth set (held-out items) of a full
    ranking.  `rowptr` int64 [n_rows + 1] and `colidx` int32 on the device; stored ids minus `col_offset` are item ids in
    [0, n_items).  Ids are ascending within every row (the kernels walk them with a cursor / binary search)."""

    def __init__(self, rowptr: torch.Tensor, colidx: torch.Tensor, col_offset: int, n_items: int, keep_alive=()):
        self.rowptr, self.colidx = rowptr, colidx
        self.col_offset, self.n_items = int(col_offset), int(n_items)
        self.n_rows = int(rowptr.numel()) - 1
        self._keep = keep_alive

    @classmethod
    def from_pairs(cls, users: torch.Tensor, items: torch.Tensor, n_user: int, n_item: int) -> "ItemSets":
        """From (user, item) pairs in any order, duplicates allowed: a sort and unique on the pairs' device (set-up, not hot path)."""
        users = users.reshape(-1).to(torch.int64)
        items = items.reshape(-1).to(device=users.device, dtype=torch.int64)
        if users.numel() != items.numel():
            raise RuntimeError("ItemSets.from_pairs: users and items differ in length")
        if users.numel() and (int(users.min()) < 0 or int(users.max()) >= n_user or int(items.min()) < 0 or int(items.max()) >= n_item):
            raise IndexError(f"ItemSets.from_pairs: a pair lies outside {n_user} users x {n_item} items")
        key = torch.unique(users * n_item + items)                   # sorted by (user, item), de-duplicated
        u, i = key // n_item, key % n_item
        rowptr = torch.zeros(n_user + 1, dtype=torch.int64, device=users.device)
        rowptr[1:] = torch.cumsum(torch.bincount(u, minlength=n_user), 0)
        return cls(rowptr, i.to(torch.int32).contiguous(), 0, n_item)

    @classmethod
    def from_laplacian(cls, csr: LaplacianCSR, n_user: int) -> "ItemSets":
        """The user rows of a model's Laplacian CSR (`model.laplacian_csr(year)`): row u holds columns n_user + item, so with
        col_offset = n_user they are the user's training items, borrowed with no copy.  The CSR's column array is never
        reordered after it is built (the swept plan keeps its own arrays), so the check below holds for the CSR's life."""
        lib = _lib.load()
        n_item = csr.n_cols - n_user
        if csr.n_rows < n_user or n_item < 1:
            raise RuntimeError(f"ItemSets.from_laplacian: a CSR of {csr.n_rows} x {csr.n_cols} has no {n_user} user rows")
        rp_ptr, ci_ptr = int(lib.ngcf_csr_rowptr(csr._h) or 0), int(lib.ngcf_csr_colidx(csr._h) or 0)
        rowptr_all = _device_view(rp_ptr, csr.n_rows + 1, torch.int64)
        nnz_user = int(rowptr_all[n_user])
        rowptr = rowptr_all[:n_user + 1]
        colidx = _device_view(ci_ptr, max(nnz_user, 1), torch.int32)[:nnz_user]
        if nnz_user > 1:
            row_of = torch.repeat_interleave(torch.arange(n_user, device=rowptr.device), rowptr.diff())
            same_row = row_of[1:] == row_of[:-1]
            if bool((same_row & (colidx[1:] < colidx[:-1])).any()):
                raise RuntimeError("ItemSets.from_laplacian: the CSR's columns are not ascending within its user rows")
        return cls(rowptr, colidx, n_user, n_item, keep_alive=(csr,))


class _DevView:
    """`__cuda_array_interface__` carrier over library-owned device memory (as dist._DevMem)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(n),), "typestr": typestr, "version": 2}


def _device_view(ptr: int, n: int, dtype) -> torch.Tensor:
    """A torch tensor over `n` elements of library-owned device memory (no copy; the owner must outlive it)."""
    if ptr == 0:
        raise RuntimeError("null device pointer")
    return torch.as_tensor(_DevView(ptr, n, {torch.int64: "<i8", torch.int32: "<i4"}[dtype]),
                           device=torch.device("cuda", torch.cuda.current_device()))


def _check_sets(s: "ItemSets", dev, n_user_rows: int, what: str):
    if s.rowptr.device != dev or s.colidx.device != dev:
        raise RuntimeError(f"{what}: the item sets live on {s.rowptr.device}, the embeddings on {dev}")
    if s.n_rows < n_user_rows:
        raise RuntimeError(f"{what}: {s.n_rows} rows of item sets for {n_user_rows} users")


def rank_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, user_ids: Optional[torch.Tensor] = None,
              exclude: Optional[ItemSets] = None, status: Optional[torch.Tensor] = None):
    """Top-k items of every item for every requested user, without a score matrix (ngcf_rank_topk_f32): fp32 MFMA scores with
    the bits of `recommend_topk`, a streaming selection per user, the user's `exclude` items left out.  With `user_ids`, batch row b
    ranks user_emb[user_ids[b]] (no gather); otherwise row b.  Returns (values [B, k], int64 indices [B, k]); slots past the
    eligible items are (-inf, -1).  Strided views (rows of all_E) are taken as they are.  A user id outside the table raises
    IndexError (one host sync); with a caller's int32 `status` word it is only flagged there and the call does not sync."""
    lib = _lib.load()
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    if user_emb.dim() != 2 or item_emb.dim() != 2 or user_emb.shape[1] != item_emb.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(user_emb.shape)} and {tuple(item_emb.t().shape)})")
    n_rows, D, n_items = int(user_emb.shape[0]), int(user_emb.shape[1]), int(item_emb.shape[0])
    k = int(k)
    if k < 1 or k > n_items:
        raise RuntimeError(f"selected index k out of range (k={k}, row length {n_items})")
    if k > RANK_K_MAX:
        raise RuntimeError(f"rank_topk: k={k} > {RANK_K_MAX} is not supported; recommend_topk takes k up to 1024")
    dev = user_emb.device
    user_emb = user_emb if user_emb.stride(1) == 1 else user_emb.contiguous()
    item_emb = item_emb if item_emb.stride(1) == 1 else item_emb.contiguous()
    if user_ids is not None:
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        B = int(user_ids.numel())
    else:
        B = n_rows
    if exclude is not None:
        _check_sets(exclude, dev, n_rows, "rank_topk")
        if exclude.n_items != n_items:
            raise RuntimeError(f"rank_topk: the exclusion sets index {exclude.n_items} items, the item table has {n_items}")
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    if B == 0:
        return vals, idx
    nb = int(lib.ngcf_rank_workspace_bytes(B, n_items, D, k))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_rank_topk_f32(_ptr(user_emb), _row_major_ld(user_emb, "user_emb"), _ptr(user_ids), n_rows, B,
                                          _ptr(item_emb), _row_major_ld(item_emb, "item_emb"), n_items, D, k,
                                          _ptr(None if exclude is None else exclude.rowptr),
                                          _ptr(None if exclude is None else exclude.colidx),
                                          0 if exclude is None else exclude.col_offset, _ptr(vals), _ptr(idx), _ptr(status),
                                          _ptr(ws), nb, _stream()))
    if check_status and user_ids is not None and int(status.item()) != 0:
        raise IndexError(f"rank_topk: a user id lies outside [0, {n_rows})")
    return vals, idx


def ranking_metrics(top_idx: torch.Tensor, truth: ItemSets, ks: Sequence[int], user_ids: Optional[torch.Tensor] = None,
                    sums: Optional[torch.Tensor] = None, per_user: bool = False, status: Optional[torch.Tensor] = None):
    """Recall / NDCG / precision / hit rate @K of top lists `top_idx` [B, k] (int64, -1 = empty slot) against `truth`
    (ngcf_rank_metrics).  Batch row b is user user_ids[b] (or b).  Users with an empty truth row are not evaluated.
    Returns {"recall@K": mean, "ndcg@K": ..., "precision@K": ..., "hr@K": ..., "users": n}.  With `sums` (a float64 device
    tensor of 4*len(ks) + 1 slots) the call adds into it and returns it instead - chunks of one ranking read back once."""
    lib = _lib.load()
    _require_device(top_idx, "top_idx")
    if top_idx.dim() != 2 or top_idx.dtype != torch.int64:
        raise RuntimeError("ranking_metrics: top_idx must be a 2-D int64 tensor")
    ks = [int(x) for x in ks]
    B, k = int(top_idx.shape[0]), int(top_idx.shape[1])
    if not ks or len(ks) > 8 or min(ks) < 1 or max(ks) > k:
        raise RuntimeError(f"ranking_metrics: between 1 and 8 cut-offs in [1, {k}], got {ks}")
    dev = top_idx.device
    top_idx = top_idx.contiguous()
    _check_sets(truth, dev, 0, "ranking_metrics")
    if user_ids is not None:
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        if int(user_ids.numel()) != B:
            raise RuntimeError("ranking_metrics: user_ids and top_idx differ in length")
    elif truth.n_rows < B:
        raise RuntimeError(f"ranking_metrics: {truth.n_rows} truth rows for {B} users")
    n_slots = 4 * len(ks) + 1
    own = sums is None
    if own:
        sums = torch.zeros(n_slots, dtype=torch.float64, device=dev)
    elif sums.dtype != torch.float64 or sums.numel() != n_slots or sums.device != dev or not sums.is_contiguous():
        raise RuntimeError(f"ranking_metrics: sums must be a contiguous float64 tensor of {n_slots} slots on {dev}")
    pu = torch.empty((B, 4 * len(ks)), dtype=torch.float32, device=dev) if per_user else None
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    ks_arr = (C.c_int32 * len(ks))(*ks)
    with _on(dev):
        _lib.check(lib.ngcf_rank_metrics(_ptr(top_idx), B, k, _ptr(user_ids), truth.n_rows, _ptr(truth.rowptr), _ptr(truth.colidx),
                                         truth.col_offset, ks_arr, len(ks), _ptr(pu), _ptr(sums), _ptr(status), _stream()))
    if check_status and user_ids is not None and int(status.item()) != 0:
        raise IndexError(f"ranking_metrics: a user id lies outside [0, {truth.n_rows})")
    if not own:
        return (sums, pu) if per_user else sums
    out = metrics_from_sums(sums, ks)
    return (out, pu) if per_user else out


def metrics_from_sums(sums: torch.Tensor, ks: Sequence[int]) -> dict:
    """The means of a `ranking_metrics` slot vector (one read-back)."""
    s = sums.double().cpu().tolist()
    n = int(round(s[-1]))
    out = {}
    for q, K in enumerate(ks):
        for j, name in enumerate(("recall", "ndcg", "precision", "hr")):
            out[f"{name}@{K}"] = s[4 * q + j] / n if n else 0.0
    out["users"] = n
    return out


# ---- candidate-list evaluation, the reference's test protocol (ngcf_eval_candidates_f32, csrc/eval_candidates.hip) ----------------
CAND_MAX = 1024


def _cand_cutoffs(ks: Sequence[int], hit_k: int, C: int):
    ks, hit_k = [int(x) for x in ks], int(hit_k)
    if len(ks) > 8:
        raise ValueError(f"eval_candidates: at most 8 NDCG cut-offs, got {len(ks)}")
    for k in ks + [hit_k]:
        if k < 1 or k > C:
            raise RuntimeError(f"selected index k out of range (k={k}, row length {C})")
    return ks, hit_k


def eval_candidates(user_emb: torch.Tensor, item_emb: torch.Tensor, user_ids: torch.Tensor, candidates: torch.Tensor,
                    ratings: Optional[torch.Tensor] = None, ks: Sequence[int] = (10,), hit_k: int = 3, weight_decay: float = 0.0,
                    batch_size: float = 1.0, user_repeat: Optional[int] = None, sums: Optional[torch.Tensor] = None,
                    status: Optional[torch.Tensor] = None, return_scores: bool = False, return_position: bool = True):
    """The reference's test protocol (experiment.py:92-116) for T cases x C candidates in one launch (ngcf_eval_candidates_f32):
    case t scores user_emb[user_ids[t]] against item_emb[candidates[t, :]], column 0 the held-out item.  `user_ids` int64 [T],
    `candidates` int64 [T, C] (C <= 1024), `ratings` float32 [T] or None, all on the embeddings' device; strided views (rows of
    all_E) are taken as they are.  Adds [hits@hit_k, ndcg@ks.., bpr sum, |s_0 - rating| sum, cases] into `sums` (float64,
    len(ks) + 4 slots; a fresh one if None) in a fixed order - see `candidate_metrics_from_sums`.  `user_repeat` (1 or C, default C)
    is how often the user row counts in the BPR regulariser.  Returns (sums, position int32 [T] or None, scores [T, C] or None);
    position = the number of candidates that sort above column 0 (ties: column 0 wins), -1 for a case with an id out of range.
    Such a case adds nothing; it raises IndexError (one host sync), or with a caller's int32 `status` word is only flagged there."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    if user_emb.dim() != 2 or item_emb.dim() != 2 or user_emb.shape[1] != item_emb.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(user_emb.shape)} and {tuple(item_emb.t().shape)})")
    for t, nm in ((user_ids, "user_ids"), (candidates, "candidates")):
        if t.dtype != torch.int64:
            raise TypeError(f"eval_candidates: {nm} must be int64, got {t.dtype}")
    if user_ids.dim() != 1 or candidates.dim() != 2 or candidates.shape[0] != user_ids.shape[0]:
        raise ValueError(f"eval_candidates: user_ids [T] and candidates [T, C] expected, got {tuple(user_ids.shape)} and {tuple(candidates.shape)}")
    T, n_cand = int(candidates.shape[0]), int(candidates.shape[1])
    if n_cand < 1 or n_cand > CAND_MAX:
        raise ValueError(f"eval_candidates: C={n_cand} candidates per case outside [1, {CAND_MAX}]")
    ks, hit_k = _cand_cutoffs(ks, hit_k, n_cand)
    user_repeat = n_cand if user_repeat is None else int(user_repeat)
    if user_repeat not in (1, n_cand):
        raise ValueError(f"eval_candidates: user_repeat={user_repeat} is neither 1 nor C={n_cand}")
    if float(batch_size) == 0.0:
        raise ValueError("eval_candidates: batch_size must not be 0")
    if ratings is not None and (ratings.dim() != 1 or int(ratings.numel()) != T):
        raise ValueError(f"eval_candidates: {tuple(ratings.shape)} ratings for {T} cases")
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    dev = user_emb.device
    if ratings is not None:
        ratings = _f32c(ratings, "ratings").contiguous()
    for t, nm in ((user_ids, "user_ids"), (candidates, "candidates"), (ratings, "ratings")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"eval_candidates: {nm} is on {t.device}, the embeddings on {dev}")
    user_emb = user_emb if user_emb.stride(1) == 1 else user_emb.contiguous()
    item_emb = item_emb if item_emb.stride(1) == 1 else item_emb.contiguous()
    user_ids = user_ids.contiguous()
    candidates = candidates if candidates.stride(1) == 1 else candidates.contiguous()
    n_slots = len(ks) + 4
    if sums is None:
        sums = torch.zeros(n_slots, dtype=torch.float64, device=dev)
    elif sums.dtype != torch.float64 or sums.numel() != n_slots or sums.device != dev or not sums.is_contiguous():
        raise ValueError(f"eval_candidates: sums must be a contiguous float64 tensor of {n_slots} slots on {dev}")
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.device != dev:
        raise ValueError(f"eval_candidates: status must be an int32 tensor on {dev}")
    scores = torch.empty((T, n_cand), dtype=torch.float32, device=dev) if return_scores else None
    position = torch.empty((T,), dtype=torch.int32, device=dev) if return_position else None
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    with _on(dev):
        _lib.check(lib.ngcf_eval_candidates_f32(
            _ptr(user_emb), _row_major_ld(user_emb, "user_emb"), int(user_emb.shape[0]), _ptr(item_emb),
            _row_major_ld(item_emb, "item_emb"), int(item_emb.shape[0]), int(user_emb.shape[1]), _ptr(user_ids), _ptr(candidates),
            _row_major_ld(candidates, "candidates"), T, n_cand, _ptr(ratings), ks_arr, len(ks), hit_k, float(weight_decay),
            float(batch_size), user_repeat, _ptr(scores), _ptr(position), _ptr(sums), _ptr(status), _stream()))
    if check_status and int(status.item()) != 0:
        raise IndexError(f"eval_candidates: a user id lies outside [0, {int(user_emb.shape[0])}) or a candidate outside "
                         f"[0, {int(item_emb.shape[0])})")
    return sums, position, scores


def candidate_metrics_from_sums(sums, ks: Sequence[int], hit_k: int = 3) -> dict:
    """The means of an `eval_candidates` slot vector [hits, ndcg@ks.., bpr, abs_err, cases] (one read-back): {"bpr", "hr@<hit_k>",
    "ndcg@K".., "rmse", "cases"}, every entry its sum over `cases` - the reference's mean over len(test_dataloader),
    experiment.py:119 ("rmse" is the mean of the per-case sqrt(MSE) of two scalars, i.e. of |s_0 - rating|)."""
    ks = [int(x) for x in ks]
    s = torch.as_tensor(sums).double().cpu().tolist()
    if len(s) != len(ks) + 4:
        raise ValueError(f"candidate_metrics_from_sums: {len(s)} slots for {len(ks)} cut-offs ({len(ks) + 4} expected)")
    n = int(round(s[-1]))
    mean = lambda x: x / n if n else 0.0   # noqa: E731
    out = {"bpr": mean(s[len(ks) + 1]), f"hr@{int(hit_k)}": mean(s[0])}
    for q, K in enumerate(ks):
        out[f"ndcg@{K}"] = mean(s[1 + q])
    out["rmse"] = mean(s[len(ks) + 2])
    out["cases"] = n
    return out


# ---- unseen items per case, the reference's TourDataset._negative_sampling (ngcf_sample_unseen, csrc/sample.hip) -------------------
SAMPLE_M_MAX = 1023


def sample_unseen(seen: ItemSets, user_ids: torch.Tensor, m: int, seed: int, *, first: Optional[torch.Tensor] = None,
                  case_offset: int = 0, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`m` items per case that the case's user has no entry for in `seen`, uniform and without replacement (ngcf_sample_unseen):
    case t of user `user_ids[t]` (int64 [T] on the sets' device) is a pure function of (seed, case_offset + t, the user's seen row)
    - the draw is written out in include/ngcf_hip.h, so a case set drawn in chunks with `case_offset` equals the set drawn at
    once.  This is the distribution of the reference's `np.random.choice(neg_items, ng_ratio, replace=False)` (utils.py:262), not
    numpy's stream: the same seed does not give the reference's items.  Returns int64 [T, m], or [T, m + 1] with `first` (int64 [T],
    e.g. the held-out items) in column 0 - then the `candidates` of `eval_candidates`.  `out`: an int64 row-major tensor of T rows
    and at least that many columns to write into (the returned tensor is a view of its leading columns).  `seen` comes from
    `ItemSets.from_pairs` or `ItemSets.from_laplacian`.  A user id outside the sets raises IndexError, a user with fewer than `m`
    unseen items ValueError (np.random.choice raises there), after one host sync; the drawn slots of such a case are -1.  With a
    caller's int32 `status` word the bits (1, 2) are only OR-ed into it and the call neither syncs nor raises."""
    lib = _lib.load()
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    if m < 1 or m > SAMPLE_M_MAX:
        raise ValueError(f"sample_unseen: m={m} outside [1, {SAMPLE_M_MAX}]")
    if seen.n_items < 1 or seen.n_items >= 2 ** 31:
        raise ValueError(f"sample_unseen: n_items={seen.n_items} outside [1, 2^31)")
    for t, nm in ((user_ids, "user_ids"), (first, "first"), (out, "out")):
        if t is not None and t.dtype != torch.int64:
            raise TypeError(f"sample_unseen: {nm} must be int64, got {t.dtype}")
    if user_ids.dim() != 1:
        raise ValueError(f"sample_unseen: user_ids must be [T], got {tuple(user_ids.shape)}")
    T = int(user_ids.numel())
    if first is not None and (first.dim() != 1 or int(first.numel()) != T):
        raise ValueError(f"sample_unseen: first must be [T = {T}], got {tuple(first.shape)}")
    width = m + (first is not None)
    if out is not None and (out.dim() != 2 or int(out.shape[0]) != T or int(out.shape[1]) < width):
        raise ValueError(f"sample_unseen: out must be [T = {T}, >= {width}], got {tuple(out.shape)}")
    _require_device(seen.rowptr, "the item sets")
    dev = seen.rowptr.device
    _check_sets(seen, dev, 0, "sample_unseen")
    if seen.rowptr.dtype != torch.int64 or seen.colidx.dtype != torch.int32:
        raise TypeError("sample_unseen: the item sets must be int64 row pointers and int32 columns")
    for t, nm in ((user_ids, "user_ids"), (first, "first"), (out, "out"), (status, "status")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"sample_unseen: {nm} is on {t.device}, the item sets on {dev}")
    if status is not None and status.dtype != torch.int32:
        raise ValueError(f"sample_unseen: status must be an int32 tensor on {dev}")
    user_ids = user_ids.contiguous()
    first = None if first is None else first.contiguous()
    if out is None:
        out = torch.empty((T, width), dtype=torch.int64, device=dev)
    ld_out = _row_major_ld(out, "out")
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    # a set without entries has no column array to point at; its row pointers are all 0 and nothing is read through it
    colidx = seen.colidx if seen.colidx.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_sample_unseen(_ptr(seen.rowptr), _ptr(colidx), seen.col_offset, seen.n_rows, seen.n_items, _ptr(user_ids), T,
                                          int(case_offset), m, seed, _ptr(first), _ptr(out), ld_out, _ptr(status), _stream()))
    if check_status and T:
        bits = int(status.item())
        if bits & 1:
            raise IndexError(f"sample_unseen: a user id lies outside [0, {seen.n_rows})")
        if bits & 2:
            raise ValueError(f"sample_unseen: a user has fewer than m={m} unseen items among {seen.n_items}")
    return out[:, :width]


# ---- per-segment quantile floor, the core of the reference's Preprocess.scale_implicit (ngcf_segment_quantile_floor_f64, csrc/quantile.hip)
QUANTILE_WAVE_MAX = 64


def segments_from_ids(ids: torch.Tensor, n_rows: int):
    """Group positions by id: `(rowptr int64 [n_rows + 1], order int64 [T])` with segment u = order[rowptr[u] : rowptr[u + 1]], the
    positions t with ids[t] == u in ascending order - the `rowptr` / `order` of `segment_quantile_floor`.  One stable `torch.sort`
    plus `bincount` and `cumsum` on the ids' device (set-up, as `ItemSets.from_pairs`); an id with no position gets an empty
    segment.  An id outside [0, n_rows) raises IndexError."""
    if ids.dim() != 1:
        raise ValueError(f"segments_from_ids: ids must be [T], got {tuple(ids.shape)}")
    if ids.dtype != torch.int64:
        raise TypeError(f"segments_from_ids: ids must be int64, got {ids.dtype}")
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError(f"segments_from_ids: n_rows={n_rows}")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_rows):
        raise IndexError(f"segments_from_ids: an id lies outside [0, {n_rows})")
    order = torch.sort(ids, stable=True).indices
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=ids.device)
    if n_rows:
        rowptr[1:] = torch.cumsum(torch.bincount(ids, minlength=n_rows), 0)
    return rowptr, order


def segment_quantile_floor(rowptr: torch.Tensor, x: torch.Tensor, *, order: Optional[torch.Tensor] = None, mean: float = 0.0,
                           scale: float = 1.0, shift: float = 0.0, q: float = 0.25, wave_max: int = 0,
                           out: Optional[torch.Tensor] = None, quant: Optional[torch.Tensor] = None,
                           status: Optional[torch.Tensor] = None):
    """Per segment u = order[rowptr[u] : rowptr[u + 1]] (positions into `x`; `order` None: x is already grouped): the `q` quantile
    of z = ((x - mean) / scale) + shift the way pandas' `quantile(q)` / numpy's `percentile(method="linear")` compute it, and every
    z below it set to 0 (ngcf_segment_quantile_floor_f64; the formulae are in include/ngcf_hip.h).  fp64 throughout, every operation
    rounded once: bit-equal to numpy up to the sign of a zero.  `rowptr` int64 [n_rows + 1], `x` float64 [T], `order` int64 [T] on one
    device.  Returns `(out float64 [T] in the order of x, quant float64 [n_rows])`; the quantile of an empty segment is NaN.  `out`
    may be `x` itself.  `q` is 0.25, 0.5 or 0.75.  `wave_max` (0: the default, 64) moves the switch between the kernel's two tiers
    and never the result.  A NaN in a segment sets status bit 2: the segment's quantile is NaN and its z pass through unfloored.
    A rowptr that decreases or leaves [0, T], or an order entry outside [0, T), sets bit 1 and leaves that segment's `out`
    unwritten: IndexError after one host sync - or, with a caller's int32 `status` word, the bits are only OR-ed into it and the
    call neither syncs nor raises."""
    lib = _lib.load()
    q4 = {0.25: 1, 0.5: 2, 0.75: 3}.get(float(q))
    if q4 is None:
        raise ValueError(f"segment_quantile_floor: q={q} is not one of 0.25, 0.5, 0.75")
    wave_max = int(wave_max)
    if wave_max < 0 or wave_max > QUANTILE_WAVE_MAX:
        raise ValueError(f"segment_quantile_floor: wave_max={wave_max} outside [0, {QUANTILE_WAVE_MAX}]")
    mean, scale, shift = float(mean), float(scale), float(shift)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"segment_quantile_floor: scale={scale} is not a finite positive number")
    for t, nm in ((rowptr, "rowptr"), (order, "order")):
        if t is not None and t.dtype != torch.int64:
            raise TypeError(f"segment_quantile_floor: {nm} must be int64, got {t.dtype}")
    for t, nm in ((x, "x"), (out, "out"), (quant, "quant")):
        if t is not None and t.dtype != torch.float64:
            raise TypeError(f"segment_quantile_floor: {nm} must be float64, got {t.dtype}")
    if rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError(f"segment_quantile_floor: rowptr must be [n_rows + 1], got {tuple(rowptr.shape)}")
    if x.dim() != 1:
        raise ValueError(f"segment_quantile_floor: x must be [T], got {tuple(x.shape)}")
    n_rows, T = int(rowptr.numel()) - 1, int(x.numel())
    for t, nm, n, sym in ((order, "order", T, "T"), (out, "out", T, "T"), (quant, "quant", n_rows, "n_rows")):
        if t is not None and (t.dim() != 1 or int(t.numel()) != n):
            raise ValueError(f"segment_quantile_floor: {nm} must be [{sym} = {n}], got {tuple(t.shape)}")
    _require_device(x, "x")
    dev = x.device
    for t, nm in ((rowptr, "rowptr"), (order, "order"), (out, "out"), (quant, "quant"), (status, "status")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"segment_quantile_floor: {nm} is on {t.device}, x on {dev}")
    if status is not None and status.dtype != torch.int32:
        raise ValueError(f"segment_quantile_floor: status must be an int32 tensor on {dev}")
    for t, nm in ((x, "x"), (out, "out"), (quant, "quant")):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"segment_quantile_floor: {nm} must be contiguous")
    rowptr = rowptr.contiguous()
    order = None if order is None else order.contiguous()
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=dev)
    if quant is None:
        quant = torch.empty(n_rows, dtype=torch.float64, device=dev)
    if T == 0:
        quant.fill_(float("nan"))                  # the library does nothing without values: every segment is empty
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_segment_quantile_floor_f64(_ptr(rowptr), n_rows, _ptr(order), _ptr(x), T, mean, scale, shift, q4, wave_max,
                                                       _ptr(quant), _ptr(out), _ptr(status), _stream()))
    if check_status and T and n_rows and int(status.item()) & 1:
        raise IndexError(f"segment_quantile_floor: a segment's row pointers or order entries lie outside the {T} values")
    return out, quant


# ---- Yeo-Johnson power transform, the core of the reference's scaler='power' (ngcf_yeo_johnson_*_f64, csrc/yeo_johnson.hip) ----------
def yeo_johnson_launch(T: int):
    """`(blocks, threads, max_blocks)` of the moments kernel's first launch for a column of T rows (a function of T alone, which is
    what makes the reduction reproducible): a grid stride is blocks * threads rows, the workspace one partial per block."""
    blocks, threads, cap = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_yeo_johnson_moments_launch(int(T), C.byref(blocks), C.byref(threads), C.byref(cap)))
    return blocks.value, threads.value, cap.value


def _yeo_johnson_args(fn: str, x: torch.Tensor, lam) -> float:
    lam = float(lam)
    if lam != lam:
        raise ValueError(f"{fn}: lam is NaN")
    if x.dtype != torch.float64:
        raise TypeError(f"{fn}: x must be float64, got {x.dtype}")
    if x.dim() != 1:
        raise ValueError(f"{fn}: x must be [T], got {tuple(x.shape)}")
    _require_device(x, "x")
    if not x.is_contiguous():
        raise ValueError(f"{fn}: x must be contiguous")
    return lam


def yeo_johnson(x: torch.Tensor, lam: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """psi(x, lam) elementwise, sklearn's `_yeo_johnson_transform` operation for operation in fp64 (ngcf_yeo_johnson_f64; the
    formulae are in include/ngcf_hip.h): `x` float64 [T] on the device, the result float64 [T].  `out` may be `x` itself.  A NaN
    passes through."""
    lib = _lib.load()
    lam = _yeo_johnson_args("yeo_johnson", x, lam)
    T = int(x.numel())
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=x.device)
    else:
        if out.dtype != torch.float64:
            raise TypeError(f"yeo_johnson: out must be float64, got {out.dtype}")
        if out.dim() != 1 or int(out.numel()) != T:
            raise ValueError(f"yeo_johnson: out must be [T = {T}], got {tuple(out.shape)}")
        if out.device != x.device:
            raise RuntimeError(f"yeo_johnson: out is on {out.device}, x on {x.device}")
        if not out.is_contiguous():
            raise ValueError("yeo_johnson: out must be contiguous")
    with _on(x.device):
        _lib.check(lib.ngcf_yeo_johnson_f64(_ptr(x), T, lam, _ptr(out), _stream()))
    return out


def yeo_johnson_moments(x: torch.Tensor, lam: float) -> torch.Tensor:
    """One evaluation of the likelihood that fits the Yeo-Johnson lambda, in one fused pass over `x` (float64 [T] on the device):
    a float64 [4] tensor on the device holding, over the rows that are not NaN, their count n, the mean of psi(x, lam),
    M2 = sum (psi - mean)^2 and c = sum sign(x) log1p|x| (ngcf_yeo_johnson_moments_f64).  Bit-identical from call to call."""
    lib = _lib.load()
    lam = _yeo_johnson_args("yeo_johnson_moments", x, lam)
    T = int(x.numel())
    result = torch.empty(4, dtype=torch.float64, device=x.device)
    nbytes = int(lib.ngcf_yeo_johnson_workspace_bytes(T))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=x.device)
    with _on(x.device):
        _lib.check(lib.ngcf_yeo_johnson_moments_f64(_ptr(x), T, lam, _ptr(result), _ptr(ws), nbytes, _stream()))
    return result


# ---- rank-point blending, the reference's recommender after its topk (ngcf_blend_points, csrc/blend.hip) ---------------------------
BLEND_TOP_MAX = 256
BLEND_POINTS_MAX = 1024


def blend_points(pref: torch.Tensor, col_rowptr: torch.Tensor, col_rows: torch.Tensor, n_items: int, *, points: int = 100,
                 weights: Sequence[float] = (1.0, 0.0, 0.0), con: Optional[torch.Tensor] = None,
                 con_slot: Optional[torch.Tensor] = None, dis: Optional[torch.Tensor] = None,
                 dis_slot: Optional[torch.Tensor] = None, item_mask: Optional[torch.Tensor] = None, top: int = 10,
                 tile_items: int = 0, return_table: bool = False, status: Optional[torch.Tensor] = None):
    """The rank-point blending of demo.py:285-292, 315-334, 378-398 for R request rows in G columns in one launch
    (ngcf_blend_points).  `pref` int64 [R, Pl]: the preference list of every request row, best first (`rank_topk`'s indices; -1 =
    empty slot); `con` int64 [S_con, Pl] with `con_slot` int64 [R] (the list of row r is con[con_slot[r]]) and `dis` / `dis_slot`
    likewise, or None for no points of that kind (`topk_rows(-values, Pl)`'s indices).  Position j of a list is worth `points` - j.
    Column g is the set of rows col_rows[col_rowptr[g]:col_rowptr[g + 1]] (int64 CSR).  Per column and item the three kinds of
    points are summed over the rows (int32, exact) and rating = (sp * w_pref + sc * w_con) + sd * w_dis in fp64 without FMA - the
    bits numpy gives.  Returns (items int64 [G, top], rating float64 [G, top]): per column the best `top` items with
    `item_mask[i] != 0` (uint8 / bool [n_items], None: all), rating descending, ties lowest item first, (-1, -inf) past the
    eligible items; with `return_table` also the dense float64 [G, n_items] ratings (tests and small catalogues only).  The result
    does not depend on `tile_items` (items per workgroup, 0 = default).  An id out of range (row index, slot, list entry, column
    range) adds nothing and raises IndexError (one host sync); with a caller's int32 `status` word it is only flagged there."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    top, points, n_items, tile_items = int(top), int(points), int(n_items), int(tile_items)
    if top < 1 or top > BLEND_TOP_MAX:
        raise ValueError(f"blend_points: top={top} outside [1, {BLEND_TOP_MAX}]")
    if points < 1 or points > BLEND_POINTS_MAX:
        raise ValueError(f"blend_points: points={points} outside [1, {BLEND_POINTS_MAX}]")
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"blend_points: n_items={n_items} outside [1, 2^31)")
    if len(weights) != 3:
        raise ValueError("blend_points: weights = (w_pref, w_con, w_dis)")
    if (con is None) != (con_slot is None) or (dis is None) != (dis_slot is None):
        raise ValueError("blend_points: a context list table and its slot vector come together")
    ints = (("pref", pref), ("col_rowptr", col_rowptr), ("col_rows", col_rows), ("con", con), ("con_slot", con_slot), ("dis", dis),
            ("dis_slot", dis_slot))
    for nm, t in ints:
        if t is not None and t.dtype != torch.int64:
            raise TypeError(f"blend_points: {nm} must be int64, got {t.dtype}")
    if item_mask is not None and item_mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"blend_points: item_mask must be uint8 or bool, got {item_mask.dtype}")
    if pref.dim() != 2 or pref.shape[1] < 1 or pref.shape[1] > points:
        raise ValueError(f"blend_points: pref must be [R, Pl] with 1 <= Pl <= points = {points}, got {tuple(pref.shape)}")
    R, Pl = int(pref.shape[0]), int(pref.shape[1])
    if R * points >= 2 ** 31:
        raise ValueError(f"blend_points: R * points = {R} * {points} >= 2^31: the int32 point sums could overflow")
    for nm, lists, slot in (("con", con, con_slot), ("dis", dis, dis_slot)):
        if lists is not None and (lists.dim() != 2 or int(lists.shape[1]) != Pl):
            raise ValueError(f"blend_points: {nm} must be [S, Pl = {Pl}], got {tuple(lists.shape)}")
        if slot is not None and (slot.dim() != 1 or int(slot.numel()) != R):
            raise ValueError(f"blend_points: {nm}_slot must be [R = {R}], got {tuple(slot.shape)}")
    if col_rowptr.dim() != 1 or col_rowptr.numel() < 1 or col_rows.dim() != 1:
        raise ValueError(f"blend_points: col_rowptr [G + 1] and col_rows [nnz] expected, got {tuple(col_rowptr.shape)} and {tuple(col_rows.shape)}")
    if item_mask is not None and (item_mask.dim() != 1 or int(item_mask.numel()) != n_items):
        raise ValueError(f"blend_points: item_mask must be [n_items = {n_items}], got {tuple(item_mask.shape)}")
    G = int(col_rowptr.numel()) - 1
    nb = int(lib.ngcf_blend_workspace_bytes(G, n_items, top, tile_items))
    if nb < 0:
        raise ValueError(f"blend_points: tile_items={tile_items} outside [0, 4096] or too many tiles for {G} columns")
    _require_device(pref, "pref")
    dev = pref.device
    for nm, t in ints + (("item_mask", item_mask),):
        if t is not None and t.device != dev:
            raise RuntimeError(f"blend_points: {nm} is on {t.device}, pref on {dev}")
    check_status = status is None
    if check_status:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.device != dev:
        raise ValueError(f"blend_points: status must be an int32 tensor on {dev}")
    pref = pref if pref.stride(1) == 1 else pref.contiguous()
    con = None if con is None else (con if con.stride(1) == 1 else con.contiguous())
    dis = None if dis is None else (dis if dis.stride(1) == 1 else dis.contiguous())
    con_slot = None if con_slot is None else con_slot.contiguous()
    dis_slot = None if dis_slot is None else dis_slot.contiguous()
    col_rowptr, col_rows = col_rowptr.contiguous(), col_rows.contiguous()
    if item_mask is not None:
        item_mask = item_mask.contiguous().view(torch.uint8)
    items = torch.empty((G, top), dtype=torch.int64, device=dev)
    rating = torch.empty((G, top), dtype=torch.float64, device=dev)
    table = torch.empty((G, n_items), dtype=torch.float64, device=dev) if return_table else None
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    ld = lambda t, nm: 0 if t is None else _row_major_ld(t, nm)   # noqa: E731
    with _on(dev):
        _lib.check(lib.ngcf_blend_points(
            _ptr(pref), ld(pref, "pref"), R, Pl, _ptr(con), ld(con, "con"), 0 if con is None else int(con.shape[0]), _ptr(con_slot),
            _ptr(dis), ld(dis, "dis"), 0 if dis is None else int(dis.shape[0]), _ptr(dis_slot), _ptr(col_rowptr), _ptr(col_rows),
            int(col_rows.numel()), G, points, n_items, float(weights[0]), float(weights[1]), float(weights[2]), _ptr(item_mask), top,
            tile_items, _ptr(items), _ptr(rating), _ptr(table), _ptr(status), _ptr(ws), nb, _stream()))
    if check_status and int(status.item()) != 0:
        raise IndexError(f"blend_points: a row index lies outside [0, {R}), a slot outside its table, a list entry outside "
                         f"[0, {n_items}) or a column range outside col_rows")
    return (items, rating, table) if return_table else (items, rating)


# ---- year-slice Laplacians straight into CSR (ngcf_laplacian_*, csrc/laplacian.hip) --------------------------------------------------
LAPLACIAN_LONG_TABLES = 16         # long rows resolved at a time: a table of 2 * n_item words each


def laplacian_limits():
    """`(wave_limit, workgroup_limit)`: the candidate counts (state entries + new records of a user) up to which a row is resolved
    by one wave in registers, and by one workgroup in LDS; longer rows take the table path.  Compiled into the library."""
    wave, group = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_laplacian_limits(C.byref(wave), C.byref(group)))
    return int(wave.value), int(group.value)


def inverse_sqrt_degree(deg: np.ndarray) -> np.ndarray:
    """float32 d^-1/2 with inf -> 0 by the reference's exact call (matrix.py:56): numpy's float32 power is not correctly rounded, so
    the same routine on the same [N, 1] shape is the only way to the same bits.  Host work on an N-sized vector."""
    with np.errstate(divide="ignore"):
        ds = np.power(deg.astype(np.float64)[:, None], -0.5, dtype=np.float32).squeeze(1)
    ds[np.isinf(ds)] = 0.0
    return ds


def empty_laplacian_state(n_user: int, device):
    """The state of R before the first year: `(rowptr int64 [n_user + 1], item int32 [0], rating float32 [0])`."""
    return (torch.zeros(int(n_user) + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device),
            torch.empty(0, dtype=torch.float32, device=device))


def build_laplacian_year(state, userid: torch.Tensor, itemid: torch.Tensor, rating: torch.Tensor, n_user: int, n_item: int):
    """One year of `matrix.laplacian_slices` on the device (the five steps of include/ngcf_hip.h, ngcf_laplacian_*): `state` is the
    user-sorted CSR of R after the earlier years (`empty_laplacian_state` before the first), `userid` / `itemid` int64 [T] and `rating`
    float32 [T] the year's records in input order, contiguous, on one device.  Returns `(new_state, rowptr int64 [N + 1], colidx
    int32 [nnz], vals float32 [nnz])`: the slice as one [N, N] CSR, user rows then item rows.  Runs on the current stream.  Read back:
    the status word with two row counts that size the launches, the N degrees for the host's d^-1/2, and the count of zero values.
    An id outside [0, n_user) / [0, n_item) raises IndexError; such records are left out of the buckets, never read through."""
    lib = _lib.load()
    rowptr0, item0, rating0 = state
    n_user, n_item = int(n_user), int(n_item)
    for t, nm, dt in ((userid, "userid", torch.int64), (itemid, "itemid", torch.int64), (rating, "rating", torch.float32),
                      (rowptr0, "state rowptr", torch.int64), (item0, "state item", torch.int32), (rating0, "state rating", torch.float32)):
        if t.dtype != dt:
            raise TypeError(f"build_laplacian_year: {nm} must be {dt}, got {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"build_laplacian_year: {nm} must be a contiguous 1-D tensor")
    T, old_nnz, N = int(userid.numel()), int(item0.numel()), n_user + n_item
    if int(itemid.numel()) != T or int(rating.numel()) != T:
        raise ValueError("build_laplacian_year: userid, itemid and rating differ in length")
    if n_user < 0 or n_item < 0 or int(rowptr0.numel()) != n_user + 1 or int(rating0.numel()) != old_nnz:
        raise ValueError(f"build_laplacian_year: the state does not belong to {n_user} users")
    _require_device(userid, "userid")
    dev = userid.device
    for t, nm in ((itemid, "itemid"), (rating, "rating"), (rowptr0, "state rowptr"), (item0, "state item"), (rating0, "state rating")):
        if t.device != dev:
            raise RuntimeError(f"build_laplacian_year: {nm} is on {t.device}, userid on {dev}")
    nb = int(lib.ngcf_laplacian_workspace_bytes(n_user, n_item))
    if nb < 0:
        raise ValueError(f"build_laplacian_year: n_user + n_item = {N} does not fit 31 bits")
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
    bptr = torch.empty(n_user + 1, dtype=torch.int64, device=dev)
    count, b_item, b_seq, b_rating, info = i32(n_user), i32(T), i32(T), f32(T), i32(4)
    with _on(dev):
        stream = _stream()
        _lib.check(lib.ngcf_laplacian_bucket(_ptr(userid), _ptr(itemid), _ptr(rating), T, n_user, n_item, _ptr(rowptr0), _ptr(count),
                                             _ptr(bptr), _ptr(b_item), _ptr(b_seq), _ptr(b_rating), _ptr(info), _ptr(ws), nb, stream))
        bad, n_block, n_long, _ = info.tolist()
        if bad:
            raise IndexError(f"build_laplacian_year: a user id lies outside [0, {n_user}) or an item id outside [0, {n_item})")
        n_tables = min(n_long, LAPLACIAN_LONG_TABLES)
        tables = i32(n_tables * 2 * n_item) if n_tables else None
        t_item, t_rating, deg = i32(old_nnz + T), f32(old_nnz + T), i32(N)
        rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
        words = torch.zeros(2, dtype=torch.int64, device=dev)              # [0]: zero values of the slice, [1]: status
        status = words[1:].view(torch.int32)
        _lib.check(lib.ngcf_laplacian_resolve(_ptr(rowptr0), _ptr(item0), _ptr(rating0), old_nnz, _ptr(bptr), _ptr(b_item), _ptr(b_seq),
                                              _ptr(b_rating), T, n_user, n_item, n_block, n_long, _ptr(t_item), _ptr(t_rating), _ptr(deg),
                                              _ptr(rowptr), _ptr(tables), n_tables, _ptr(status), _ptr(ws), nb, stream))
        deg_host = deg.cpu().numpy()                                        # the year's one N-sized read-back
        nnz = int(deg_host[:n_user].sum(dtype=np.int64))
        ds = torch.from_numpy(inverse_sqrt_degree(deg_host)).to(dev)
        s_item, s_rating, s_user, vals_item = i32(nnz), f32(nnz), i32(nnz), f32(nnz)
        colidx, vals = i32(2 * nnz), f32(2 * nnz)
        _lib.check(lib.ngcf_laplacian_emit(_ptr(rowptr0), _ptr(item0), _ptr(rating0), old_nnz, _ptr(bptr), T, _ptr(t_item), _ptr(t_rating),
                                           n_user, n_item, _ptr(deg), _ptr(rowptr), _ptr(ds), nnz, _ptr(s_item), _ptr(s_rating), _ptr(s_user),
                                           _ptr(colidx), _ptr(vals), _ptr(vals_item), _ptr(words), _ptr(status), stream))
        del t_item, t_rating, b_item, b_seq, b_rating
        order = torch.sort(s_item, stable=True).indices                     # item rows by (item, user): one library sort of 32-bit keys
        _lib.check(lib.ngcf_laplacian_item_rows(_ptr(order), _ptr(s_user), _ptr(vals_item), nnz, _ptr(colidx[nnz:]), _ptr(vals[nnz:]),
                                                _ptr(status), stream))
        zeros, st = words.tolist()
        if st & 0xffffffff:
            raise RuntimeError(f"build_laplacian_year: the state handed in is not a CSR of {n_user} users over {n_item} items "
                               f"(status {st & 0xffffffff})")
        if zeros:                                                           # values that underflow to 0 leave the slice, not the state
            out_rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
            out_colidx, out_vals = i32(2 * nnz - zeros), f32(2 * nnz - zeros)
            _lib.check(lib.ngcf_laplacian_drop_zeros(_ptr(rowptr), _ptr(colidx), _ptr(vals), N, 2 * nnz, _ptr(deg), _ptr(out_rowptr),
                                                     _ptr(out_colidx), _ptr(out_vals), 2 * nnz - zeros, _ptr(ws), nb, stream))
            return (rowptr[:n_user + 1], s_item, s_rating), out_rowptr, out_colidx, out_vals
    return (rowptr[:n_user + 1], s_item, s_rating), rowptr, colidx, vals


# ---- group-by-sum on packed integer keys and the decimal string code (ngcf_groupby_*, ngcf_decimal_code, csrc/groupby.hip) -----------
GROUPBY_MAX_KEYS, GROUPBY_MAX_VALUES = 8, 4
GROUPBY_FULL, GROUPBY_RANGE, GROUPBY_LOST = 1, 2, 4
GROUPBY_MIN_CAPACITY = 64
GROUPBY_LDS_SLOTS = 1024           # the default `lds_slots`; profiles/groupby_lab.txt records the run that sets it (none yet)
DECIMAL_MAX_CHARS = 18


class _GroupbyCols(C.Structure):
    """ngcf_groupby_cols_t of include/ngcf_hip.h."""
    _fields_ = [("n_keys", C.c_int32), ("n_values", C.c_int32), ("key", C.c_void_p * GROUPBY_MAX_KEYS),
                ("value", C.c_void_p * GROUPBY_MAX_VALUES), ("key_offset", C.c_int64 * GROUPBY_MAX_KEYS),
                ("key_range", C.c_uint64 * GROUPBY_MAX_KEYS), ("key_is64", C.c_int32 * GROUPBY_MAX_KEYS),
                ("key_bits", C.c_int32 * GROUPBY_MAX_KEYS), ("key_shift", C.c_int32 * GROUPBY_MAX_KEYS),
                ("value_is64", C.c_int32 * GROUPBY_MAX_VALUES)]


class Groups(NamedTuple):
    """`group_by`'s result: `keys` K int64 [G] columns in ascending (column 0, column 1, ...) order, `sums` V int64 [G] columns,
    `inverse` int64 [T] (row t belongs to group inverse[t]) or None."""
    keys: Tuple[torch.Tensor, ...]
    sums: Tuple[torch.Tensor, ...]
    inverse: Optional[torch.Tensor]


def groupby_limits():
    """`(chunk_rows, lds_probes, max_lds_slots)` of the insert kernel: the rows a workgroup takes per pass, the probes a row gets in
    the workgroup's LDS table before it goes to memory, and the largest `lds_slots`.  Compiled into the library."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_groupby_limits(C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def groupby_hash(key: int) -> int:
    """The hash of a packed key (fmix64, the 64-bit finaliser of MurmurHash3): its home slot is `hash & (capacity - 1)`, its slot
    in a workgroup's LDS table `(hash >> 32) & (lds_slots - 1)`.  Host call."""
    return int(_lib.load().ngcf_groupby_hash(int(key) & (2 ** 64 - 1)))


def groupby_packing(bounds: Sequence[Tuple[int, int]]):
    """`(offsets, ranges, bits, shifts)` of key columns with the given (min, max): a field of bit_length(max - min) bits per column
    (none for a single-valued one), column 0 most significant.  More than 63 bits in all: ValueError (the all-ones word must stay
    free to mean an empty slot)."""
    offsets = [int(lo) for lo, _ in bounds]
    ranges = [int(hi) - int(lo) for lo, hi in bounds]
    if any(r < 0 for r in ranges):
        raise ValueError(f"group_by: bounds {list(bounds)}: a maximum below its minimum")
    bits = [r.bit_length() for r in ranges]
    if sum(bits) > 63:
        raise ValueError(f"group_by: the columns need {' + '.join(map(str, bits))} = {sum(bits)} bits, and a packed key has 63")
    shifts = [sum(bits[k + 1:]) for k in range(len(bits))]
    return offsets, ranges, bits, shifts


_NO_FLOAT_SUMS = ("only integer columns are summed: pandas' float group sum is compensated, so its bits cannot be met, and "
                  "floating-point atomics would make the result depend on arrival order")


def _int_columns(fn: str, groups):
    """Types and shapes of every column first (they hold on any device), then where the columns live.  `groups`: (what, columns)
    pairs; returns the columns of each, contiguous."""
    T = None
    for what, cols in groups:
        for k, c in enumerate(cols):
            if not isinstance(c, torch.Tensor):
                raise TypeError(f"{fn}: {what} {k} is not a tensor")
            if c.dtype.is_floating_point and what == "value column":
                raise TypeError(f"{fn}: {what} {k} is {c.dtype}; {_NO_FLOAT_SUMS}")
            if c.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"{fn}: {what} {k} must be int32 or int64, got {c.dtype}")
            if c.dim() != 1:
                raise ValueError(f"{fn}: {what} {k} must be [T], got {tuple(c.shape)}")
            if T is not None and int(c.numel()) != T:
                raise ValueError(f"{fn}: {what} {k} has {int(c.numel())} rows, {groups[0][0]} 0 has {T}")
            T = int(c.numel())
    dev = None
    for what, cols in groups:
        for k, c in enumerate(cols):
            _require_device(c, f"{fn}: {what} {k}")
            if dev is not None and c.device != dev:
                raise RuntimeError(f"{fn}: {what} {k} is on {c.device}, {groups[0][0]} 0 on {dev}")
            dev = c.device
    return [[c.contiguous() for c in cols] for _, cols in groups]


def group_by(columns: Sequence[torch.Tensor], values: Sequence[torch.Tensor] = (), *, inverse: bool = False,
             capacity: Optional[int] = None, lds_slots: Optional[int] = None,
             bounds: Optional[Sequence[Tuple[int, int]]] = None) -> Groups:
    """Group the T rows of `columns` (K <= 8 int32 / int64 [T] tensors on one device) by their values and sum `values` (V <= 4
    int32 / int64 [T]) per group: `pd.pivot_table(index=columns, aggfunc='sum').reset_index()`, or `np.unique(axis=0,
    return_inverse=True)` plus `np.add.at` (ngcf_groupby_*; the steps are in include/ngcf_hip.h).  Returns `Groups(keys, sums,
    inverse)`: the G distinct key rows ascending by (column 0, column 1, ...) as K int64 [G] tensors, the V int64 [G] sums (exact,
    modulo 2^64), and with `inverse=True` the int64 [T] group index of every row.  Integer atomics only: the same call returns the
    same tensors.  Floating value columns are a TypeError.  The columns' (min, max) are read back once to pack the keys into
    <= 63 bits (more: ValueError), or taken from `bounds` (K pairs; a value outside them: ValueError); G and the status word are the
    other read-back.  `capacity` (a power of two; default: the power of two >= 2 x min(T, product of the ranges), which cannot
    overflow) is doubled and the call run again while the table turns out too small; `lds_slots` (0: off; a power of two up to
    `groupby_limits()[2]`; default GROUPBY_LDS_SLOTS) sizes the per-workgroup LDS table and never changes the result."""
    lib = _lib.load()
    fn = "group_by"
    columns, values = list(columns), list(values)
    if not 1 <= len(columns) <= GROUPBY_MAX_KEYS:
        raise ValueError(f"{fn}: {len(columns)} key columns, outside [1, {GROUPBY_MAX_KEYS}]")
    if len(values) > GROUPBY_MAX_VALUES:
        raise ValueError(f"{fn}: {len(values)} value columns, more than {GROUPBY_MAX_VALUES}")
    if capacity is not None:
        capacity = int(capacity)
        if capacity < 1 or capacity & (capacity - 1) or capacity > 2 ** 36:
            raise ValueError(f"{fn}: capacity={capacity} is not a power of two in [1, 2^36]")
    lds_slots = GROUPBY_LDS_SLOTS if lds_slots is None else int(lds_slots)
    if lds_slots != 0 and (lds_slots < 16 or lds_slots & (lds_slots - 1) or lds_slots > 2048):
        raise ValueError(f"{fn}: lds_slots={lds_slots} is neither 0 nor a power of two in [16, 2048]")
    K, V = len(columns), len(values)
    if bounds is not None and len(bounds) != K:
        raise ValueError(f"{fn}: {len(bounds)} bounds for {K} columns")
    columns, values = _int_columns(fn, (("key column", columns), ("value column", values)))
    T, dev = int(columns[0].numel()), columns[0].device
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)  # noqa: E731
    if T == 0:
        return Groups(tuple(i64(0) for _ in range(K)), tuple(i64(0) for _ in range(V)), i64(0) if inverse else None)
    if bounds is None:                                                     # read-back 1: the K (min, max) pairs
        mm = torch.stack([f(c).to(torch.int64) for c in columns for f in (torch.min, torch.max)]).tolist()
        bounds = [(mm[2 * k], mm[2 * k + 1]) for k in range(K)]
    offsets, ranges, bits, shifts = groupby_packing(bounds)
    cols = _GroupbyCols()
    cols.n_keys, cols.n_values = K, V
    for k, c in enumerate(columns):
        cols.key[k], cols.key_is64[k] = c.data_ptr(), int(c.dtype == torch.int64)
        cols.key_offset[k], cols.key_range[k], cols.key_bits[k], cols.key_shift[k] = offsets[k], ranges[k], bits[k], shifts[k]
    for v, c in enumerate(values):
        cols.value[v], cols.value_is64[v] = c.data_ptr(), int(c.dtype == torch.int64)
    if capacity is None:
        prod = 1
        for r in ranges:
            prod = min(prod * (r + 1), T)                                  # min(T, product of the ranges): the most groups there can be
        capacity = max(GROUPBY_MIN_CAPACITY, 1 << (2 * prod - 1).bit_length())
    with _on(dev):
        stream = _stream()
        while True:
            table_keys, table_sums = i64(capacity), i64(max(V * capacity, 1))
            words = torch.zeros(2, dtype=torch.int64, device=dev)          # [0]: G, [1]: the status word
            status = words[1:].view(torch.int32)                           # its first int32 is the word
            nb = int(lib.ngcf_groupby_workspace_bytes(capacity))
            ws = i64(max(nb // 8, 1))
            _lib.check(lib.ngcf_groupby_insert(C.byref(cols), T, _ptr(table_keys), _ptr(table_sums), capacity, lds_slots, _ptr(status), stream))
            _lib.check(lib.ngcf_groupby_count(_ptr(table_keys), capacity, _ptr(words), _ptr(ws), nb, stream))
            G, st = words.tolist()                                         # read-back 2: G and the status word
            st &= 0xffffffff
            if st & GROUPBY_RANGE:
                raise ValueError(f"{fn}: a value lies outside the bounds {list(bounds)} its column was packed with")
            if not st & GROUPBY_FULL:
                break
            if capacity >= 2 ** 36:
                raise RuntimeError(f"{fn}: the groups do not fit a table of 2^36 slots")
            del table_keys, table_sums
            capacity *= 2
        keys_g, slots_g = i64(G), i64(G)
        _lib.check(lib.ngcf_groupby_compact(_ptr(table_keys), capacity, G, _ptr(keys_g), _ptr(slots_g), _ptr(ws), nb, _ptr(status), stream))
        sorted_keys, order = torch.sort(keys_g)                            # packed keys are below 2^63: the signed order is theirs
        key_out, sum_out = [i64(G) for _ in range(K)], [i64(G) for _ in range(V)]
        rank = i64(capacity) if inverse else None
        kp = (C.c_void_p * GROUPBY_MAX_KEYS)(*[t.data_ptr() for t in key_out])
        sp = (C.c_void_p * GROUPBY_MAX_VALUES)(*[t.data_ptr() for t in sum_out])
        _lib.check(lib.ngcf_groupby_unpack(C.byref(cols), _ptr(sorted_keys), _ptr(order), _ptr(slots_g), _ptr(table_sums), capacity, G, kp, sp,
                                           _ptr(rank), _ptr(status), stream))
        inv = None
        if inverse:
            inv = i64(T)
            _lib.check(lib.ngcf_groupby_lookup(C.byref(cols), T, _ptr(table_keys), _ptr(rank), capacity, _ptr(inv), _ptr(status), stream))
        st = int(status[0].item())                                         # the status word once more, after the last kernel
    if st:
        raise RuntimeError(f"{fn}: the columns changed while the call ran (status {st})")
    return Groups(tuple(key_out), tuple(sum_out), inv)


def decimal_code(columns: Sequence[torch.Tensor], widths: Sequence[int]) -> torch.Tensor:
    """One int64 [T] column whose numeric order is the lexicographic order of the strings `str(col0) + str(col1) + ...` (up to 8
    non-negative int32 / int64 [T] columns on one device; ngcf_decimal_code).  `widths[k] = 0`: the value's natural decimal length;
    `w > 0`: zero-padded on the left to w characters.  Every character '0' + d is the base-11 digit d + 1 of a left-aligned number
    of 18 places, padding 0 (11^18 < 2^63); `decimal_string` is the way back.  ValueError for a negative value, a value with more
    digits than its fixed width, and a string of more than 18 characters (one read-back of the status word)."""
    lib = _lib.load()
    fn = "decimal_code"
    columns, widths = list(columns), [int(w) for w in widths]
    if not 1 <= len(columns) <= GROUPBY_MAX_KEYS:
        raise ValueError(f"{fn}: {len(columns)} columns, outside [1, {GROUPBY_MAX_KEYS}]")
    if len(widths) != len(columns):
        raise ValueError(f"{fn}: {len(widths)} widths for {len(columns)} columns")
    if any(w < 0 or w > DECIMAL_MAX_CHARS for w in widths):
        raise ValueError(f"{fn}: widths {widths} outside [0, {DECIMAL_MAX_CHARS}]")
    if sum(max(w, 1) for w in widths) > DECIMAL_MAX_CHARS:
        raise ValueError(f"{fn}: widths {widths} make more than {DECIMAL_MAX_CHARS} characters")
    columns, = _int_columns(fn, (("column", columns),))
    n, T, dev = len(columns), int(columns[0].numel()), columns[0].device
    out = torch.empty(T, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in columns])
    is64 = (C.c_int32 * n)(*[int(c.dtype == torch.int64) for c in columns])
    wd = (C.c_int32 * n)(*widths)
    with _on(dev):
        _lib.check(lib.ngcf_decimal_code(ptrs, is64, wd, n, T, _ptr(out), _ptr(status), _stream()))
    st = int(status.item()) if T else 0
    if st & 1:
        raise ValueError(f"{fn}: a column holds a negative value")
    if st & 2:
        raise ValueError(f"{fn}: a value has more digits than its fixed width (widths {widths})")
    if st & 4:
        raise ValueError(f"{fn}: a row's string has more than {DECIMAL_MAX_CHARS} characters")
    return out


def decimal_string(code: int) -> str:
    """The string behind one `decimal_code` value (host, for the few distinct keys of a dictionary)."""
    code, chars = int(code), []
    if code < 0 or code >= 11 ** DECIMAL_MAX_CHARS:
        raise ValueError(f"decimal_string: {code} is not a code")
    for _ in range(DECIMAL_MAX_CHARS):
        code, d = divmod(code, 11)
        chars.append(d)
    chars.reverse()                                                        # most significant place first
    n = len(chars)
    while n and chars[n - 1] == 0:
        n -= 1
    if any(d == 0 for d in chars[:n]):
        raise ValueError("decimal_string: padding inside the string: not a code")
    return "".join(chr(ord("0") + d - 1) for d in chars[:n])


# ---- exact per-group sampling, the core of the reference's Preprocess.split_train_test (ngcf_select_per_group, csrc/select.hip) ------
SELECT_GROUP, SELECT_QUOTA, SELECT_LOST = 1, 2, 4          # the status bits of include/ngcf_hip.h
SELECT_GOLDEN = 0x9E3779B97F4A7C15


def select_limits(n_groups: int = 1):
    """`(lds_groups, workspace_bytes)`: the largest group count whose G x 256 table of counts a workgroup keeps in LDS (above it
    the rows count straight into memory), and the bytes of workspace a call with `n_groups` groups takes - 1 KiB + 16 B per group
    in both tiers (-1 for a count outside [1, 2^31)).  Compiled into the library."""
    a, b = C.c_int(0), C.c_int64(0)
    _lib.check(_lib.load().ngcf_select_limits(int(n_groups), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def select_key(seed: int, t: int) -> int:
    """The key of row t, fmix(seed ^ (t * 0x9E3779B97F4A7C15)) in unsigned 64-bit arithmetic, as the library computes it.  Host call."""
    return int(_lib.load().ngcf_select_key(int(seed) & (2 ** 64 - 1), int(t)))


def select_per_group(group: Optional[torch.Tensor], quota, *, seed: int, n_rows: Optional[int] = None, return_thresholds: bool = False,
                     out: Optional[torch.Tensor] = None, device=None):
    """Mark exactly `quota[g]` rows of every group g, uniformly among all subsets of that size (ngcf_select_per_group; the keys and
    the rule are written out in include/ngcf_hip.h): row t of group g is marked iff its key is among the quota[g] smallest of the
    group.  `group`: int32 [T] on the device, ids in [0, G), in any order - or None for one group of `n_rows` rows (on `device`,
    default the current one).  `quota`: G integers (a sequence, an array or a tensor; it is checked on the host and uploaded).
    Returns the uint8 [T] mask (0 / 1), a pure function of (seed, group, quota) - or `(mask, thresholds)` with `return_thresholds`:
    int64 [G] holding the bits of the unsigned 64-bit tau_g, 0 for a group with nothing marked.  `out`: a contiguous uint8 [T] tensor
    to write the mask into.  A negative quota is a ValueError before anything runs.  One status read-back at the end: a group id
    outside [0, G) raises IndexError (and the mask, which `out` still shows, is all 0), a quota above its group's row count
    ValueError (np.random.choice and pandas' sample raise there; no row of that group is marked).  This is the reference's
    distribution, not numpy's or pandas' stream: the same seed does not give the reference's rows."""
    lib = _lib.load()
    fn = "select_per_group"
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if group is not None:
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32:
            raise TypeError(f"{fn}: group must be an int32 tensor, got {getattr(group, 'dtype', type(group))}")
        if group.dim() != 1:
            raise ValueError(f"{fn}: group must be [T], got {tuple(group.shape)}")
        if n_rows is not None and int(n_rows) != int(group.numel()):
            raise ValueError(f"{fn}: n_rows={n_rows} beside a group vector of {int(group.numel())} rows")
        T = int(group.numel())
    else:
        if n_rows is None:
            raise ValueError(f"{fn}: without a group vector n_rows says how many rows there are")
        T = int(n_rows)
    if T < 0 or T >= 2 ** 31:
        raise ValueError(f"{fn}: {T} rows, outside [0, 2^31)")
    q = quota.detach().cpu() if isinstance(quota, torch.Tensor) else torch.as_tensor(np.asarray(quota))
    if q.dim() != 1 or q.numel() < 1:
        raise ValueError(f"{fn}: quota must be [G >= 1], got {tuple(q.shape)}")
    if q.dtype.is_floating_point or q.dtype == torch.bool:
        raise TypeError(f"{fn}: quota must hold integers, got {q.dtype}")
    q = q.to(torch.int64).contiguous()
    G = int(q.numel())
    if group is None and G != 1:
        raise ValueError(f"{fn}: no group vector stands for one group, quota has {G} entries")
    if bool((q < 0).any()):
        raise ValueError(f"{fn}: a quota is negative")
    if out is not None and (out.dtype != torch.uint8 or out.dim() != 1 or int(out.numel()) != T or not out.is_contiguous()):
        raise ValueError(f"{fn}: out must be a contiguous uint8 [T = {T}] tensor")
    if group is not None:
        _require_device(group, "group")
        dev = group.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{fn}: device '{dev}': the selection runs on a ROCm device only")
    if out is not None and out.device != dev:
        raise RuntimeError(f"{fn}: out is on {out.device}, the rows on {dev}")
    group = None if group is None else group.contiguous()
    mask = torch.empty(T, dtype=torch.uint8, device=dev) if out is None else out
    thresholds = torch.empty(G, dtype=torch.int64, device=dev) if return_thresholds else None
    quota_d = q.to(dev)
    nb = select_limits(G)[1]
    ws = torch.empty(nb // 16 * 2, dtype=torch.int64, device=dev)         # torch's allocations are 16-byte aligned and more
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_select_per_group(_ptr(group), T, G, _ptr(quota_d), seed, _ptr(mask), _ptr(thresholds), _ptr(status), _ptr(ws),
                                             nb, _stream()))
    bits = int(status.item())                                             # the one read-back
    if bits & SELECT_GROUP:
        raise IndexError(f"{fn}: a group id lies outside [0, {G})")
    if bits & SELECT_QUOTA:
        raise ValueError(f"{fn}: a quota is larger than its group's row count")
    if bits:
        raise RuntimeError(f"{fn}: the group vector changed while the call ran (status {bits})")
    return (mask, thresholds) if return_thresholds else mask
