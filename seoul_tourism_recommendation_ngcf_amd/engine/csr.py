"""The device CSR of a Laplacian slice and the host's row partition: `ngcf_csr_*` (csrc/csr.hip; the header's section "Laplacian:
COO -> CSR") and `ngcf_shard_plan` (csrc/ops.hip; "multi-GPU row partition")."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _stream


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

    def groups(self) -> list:
        """The row groups of the current plan (ngcf_csr_group; for tests and tools): one dict per group with `begin`, `end`,
        `sliceable`, `lds_table`, `col_lo`, `col_hi` (col_hi < col_lo: the group has no entries)."""
        lib = _lib.load()
        out = []
        for g in range(int(lib.ngcf_csr_n_groups(self._h))):
            b, e, s, t, lo, hi = C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_int32(), C.c_int32()
            _lib.check(lib.ngcf_csr_group(self._h, g, C.byref(b), C.byref(e), C.byref(s), C.byref(t), C.byref(lo), C.byref(hi)))
            out.append({"begin": b.value, "end": e.value, "sliceable": bool(s.value), "lds_table": bool(t.value),
                        "col_lo": lo.value, "col_hi": hi.value})
        return out

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


def shard_plan(rowptr_host: torch.Tensor, row_begin: int, row_end: int, world: int):
    """nnz-balanced contiguous cut of rows [row_begin,row_end) into `world` ranges (host helper)."""
    lib = _lib.load()
    rp = rowptr_host.to(device="cpu", dtype=torch.int64).contiguous()
    bounds = (C.c_int64 * (world + 1))()
    _lib.check(lib.ngcf_shard_plan(C.cast(rp.data_ptr(), C.POINTER(C.c_int64)), row_begin, row_end, world, bounds))
    return [int(b) for b in bounds]
