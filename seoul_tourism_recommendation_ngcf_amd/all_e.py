"""all_E, the `cat` of NGCF.py:147: how it is allocated and E0 written into it, the all_E an inference forward keeps (`E0Cache`), and
how a graph runner tells that a caller still holds its static all_E (`static_result_*`)."""
from __future__ import annotations

import sys

import torch

from . import engine as _eng


def _padded_rows(n: int, d: int, dev) -> torch.Tensor:
    """[n, d] fp32 whose rows start on 128-byte lines (leading dimension rounded up to 32 floats): the float4 / L2-swept SpMM and
    the branch-free dense path then apply at the reference's own widths too (65 -> 96)."""
    return torch.empty((n, (d + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :d]


def _final_rows(n: int, d: int, dev) -> torch.Tensor:
    """[n, d] fp32, contiguous: the gradient of the two embedding tables as autograd wants it (see Propagate.backward)."""
    return torch.empty((n, d), dtype=torch.float32, device=dev)


def _alloc_all_E(N: int, widths, dev) -> torch.Tensor:
    """all_E [N, D] for the `cat` of NGCF.py:147.  The reference forces embed_size to a multiple of 5 (NGCF.py:39-43: 65, 130,
    515), so D is usually not a multiple of 4 and contiguous rows would not be 16-byte aligned.  Then the rows are padded to a
    multiple of 32 floats (a [N, D] view of a [N, ld] buffer: every row starts on a 128-byte line), so that block 0 - E0, which the
    first layer gathers from - serves the float4 / L2-swept kernels where it lies.  (r02 wrote a second, aligned copy of E0 for
    that: 1.2 GB more traffic per forward at C3's 130-wide tables.)"""
    D = sum(widths)
    if D % 4 == 0 and widths[0] % 4 == 0:
        return torch.empty((N, D), dtype=torch.float32, device=dev)
    return torch.empty((N, (D + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :D]


def _write_e0(owner, user_w, item_w, all_E, U, d0):
    """E0 into its column block of all_E (the `cat` of NGCF.py:120 and of NGCF.py:147); returns E0 as the first layer reads it:
    block 0 itself, whose rows are 16-byte aligned in either layout of `_alloc_all_E`."""
    _eng.copy_rows(user_w.detach(), all_E[:U, :d0])
    _eng.copy_rows(item_w.detach(), all_E[U:, :d0])
    return all_E[:, :d0]


class _Probe:
    pass


def static_result_counts(all_E: torch.Tensor):
    """(Python references, C++ references, tensors on the storage) of a graph's STATIC all_E - compared with the same reading taken
    when only the graph runner held it (`GraphedForward`, `train_graphs._TrainGraphs`): anything more means a caller still holds the
    previous replay's `model.all_items_emb` / `all_users_emb` / a slice of them, and the next forward must not replay over it (the
    reference allocates a fresh all_E per call, NGCF.py:147-149)."""
    return (sys.getrefcount(all_E), all_E._use_count(), torch._C._storage_Use_Count(all_E.untyped_storage()._cdata))


def static_result_baseline(all_E: torch.Tensor):
    """The reading of `static_result_counts` for a tensor only its runner holds, taken through ONE intermediate frame - the shape of
    the later check (`_static_result_held(model, all_E, ...)` -> `static_result_counts(all_E)`): every frame that binds the tensor to
    a parameter is one more Python reference, so the two readings must come up the same call depth."""
    return static_result_counts(all_E)


def _static_result_held(model, static_all_E, free_counts) -> bool:
    """Does a caller still hold the previous replay's `all_users_emb` / `all_items_emb` / `_all_E` (or a view of them)?  They are
    views of the graph's static all_E, which the next replay overwrites - the reference hands out a fresh `cat` per call
    (NGCF.py:147-149), so a held tensor must stay what it was: then this forward runs eagerly (r04; r03 documented the
    overwrite as a deviation).  The module's own references are dropped first - both paths set them again."""
    d = model.__dict__
    if d.get("_all_E") is static_all_E or getattr(d.get("all_users_emb"), "_base", None) is static_all_E:
        d["_all_E"] = d["all_users_emb"] = d["all_items_emb"] = None
    return static_result_counts(static_all_E) != free_counts


class E0Cache:
    """The all_E of the previous inference forward, kept so that block 0 - E0 = cat(user table, item table), NGCF.py:120 - need not
    be copied again while the tables are unchanged (r04; SURVEY 2.2 K4: 563 MB through `copy_rows_kernel` per forward at C3, 0.21 ms).

    Re-used only when ALL of this holds, else a fresh all_E is allocated and E0 copied in full, exactly as before:
      * both tables are the same tensors (address, shape) at the same autograd version counter as when block 0 was written
        (optimizer steps, `load_state_dict`, `nn.init` and every other in-place op on the Parameter bump it; `.to()` moves it);
      * nobody but the module holds the old all_E or a view of it: Python reference counts of the tensor and of the module's two
        views (`all_users_emb`, `all_items_emb`) and the use count of their storage are exactly the module's own - a caller who
        kept `model.all_items_emb` (demo.py:233) or a slice of it keeps it intact, as with the reference's fresh `cat` per call
        (copy-on-hold rather than a rotation of buffers).
    The rows the feature injection rewrites through `.data` (NGCF.py:114-115 - invisible to the version counter, but done by this
    module's own kernel) are recorded (`touch`) and copied row by row.  What the cache cannot see: a write through `.data` from
    OUTSIDE the module (`.detach()`-ed aliases share the counter and are seen) - call `model.invalidate_all_E()` after such a
    write, or set `NGCF.reuse_all_E = False`."""

    MAX_TOUCHED = 8            # batches of injected rows remembered; beyond that the next forward copies everything

    def __init__(self):
        self.all_E, self.tag, self.touched = None, None, []

    def invalidate(self):
        self.all_E, self.tag, self.touched = None, None, []

    def touch(self, rows: torch.Tensor):
        """`rows` (int64, device) of the user table were rewritten in place."""
        if self.all_E is None:
            return
        if len(self.touched) >= self.MAX_TOUCHED:
            self.invalidate()
        else:
            self.touched.append(rows)

    @staticmethod
    def tag_of(user_w, item_w, widths, dev):
        return (user_w.data_ptr(), int(user_w._version), tuple(user_w.shape), item_w.data_ptr(), int(item_w._version),
                tuple(item_w.shape), tuple(widths), str(dev))

    def _counts(self, owner):
        """(Python references to all_E and to each of the module's two views, C++ references to the three tensors - a DLPack capsule
        or another extension holding one of them shows up there -, tensors on the storage) - read the same way here and in the
        calibration below, so the constants of this interpreter / torch build cancel out."""
        d = owner.__dict__
        return (sys.getrefcount(self.all_E), sys.getrefcount(d["all_users_emb"]), sys.getrefcount(d["all_items_emb"]),
                self.all_E._use_count(), d["all_users_emb"]._use_count(), d["all_items_emb"]._use_count(),
                torch._C._storage_Use_Count(self.all_E.untyped_storage()._cdata))

    _free = {}

    @classmethod
    def _free_counts(cls, padded: bool):
        """What `_counts` reads when nobody but the module and its cache holds the forward's tensors: measured once per layout of
        all_E (`_alloc_all_E`: a plain [N, D] tensor, or - D not a multiple of 4 - a [N, D] view of a padded buffer) on a toy built
        the way `NGCF.propagate` builds the real thing."""
        if padded not in cls._free:
            o, c = _Probe(), cls()
            t = torch.empty((4, 8))[:, :6] if padded else torch.empty((4, 8))
            o._all_E, o.all_users_emb, o.all_items_emb = t, t[:2, :], t[2:, :]
            c.all_E = t
            del t
            cls._free[padded] = c._counts(o)
        return cls._free[padded]

    def only_the_modules(self, owner) -> bool:
        """True iff the cached all_E and the module's two views of it are referenced by the module (and this cache) alone."""
        d = owner.__dict__
        if self.all_E is None or d.get("_all_E") is not self.all_E:
            return False
        root = self.all_E._base if self.all_E._base is not None else self.all_E
        for name in ("all_users_emb", "all_items_emb"):
            if d.get(name) is None or d[name]._base is not root:
                return False
        del root
        return self._counts(owner) == self._free_counts(self.all_E._base is not None)


def _all_E_with_e0(owner, user_w, item_w, N, widths, dev):
    """(all_E with block 0 = E0 written, E0 as the first layer reads it).  `owner._e0_cache` (NGCF modules; the graph runners
    have none): see `E0Cache`."""
    U, d0 = int(user_w.shape[0]), widths[0]
    cache = getattr(owner, "_e0_cache", None)
    if cache is not None and getattr(owner, "reuse_all_E", True) and not torch.cuda.is_current_stream_capturing():
        tag = E0Cache.tag_of(user_w, item_w, widths, dev)
        if cache.tag == tag and cache.only_the_modules(owner):
            all_E = cache.all_E
            for rows in cache.touched:
                _eng.copy_rows_indexed(user_w.detach(), all_E[:U, :d0], rows)
            cache.touched = []
            return all_E, all_E[:, :d0]
        cache.invalidate()                     # (drops the old block before the new one is allocated)
        all_E = _alloc_all_E(N, widths, dev)
        prev = _write_e0(owner, user_w, item_w, all_E, U, d0)
        cache.all_E, cache.tag = all_E, tag
        return all_E, prev
    all_E = _alloc_all_E(N, widths, dev)
    return all_E, _write_e0(owner, user_w, item_w, all_E, U, d0)
