"""Reference-mode dropout masks: torch's default CPU generator regenerated on the host, and what a forward makes of the draws.

The reference draws its node- and message-dropout masks with `nn.Dropout` on CPU tensors (NGCF.py:93-100,142).  The first half of
this module is pure host code with no dependence on the model: `_reference_bernoulli` / `_draw_program` reproduce those draws bit
for bit (through `ngcf_torch_cpu_bernoulli`, csrc/hostrng.hip, where that matches this torch build: `_host_rng_ok`), `_DrawAhead`
draws the next forward's masks on a helper thread.  The second half - `reference_draws(model, ...)` and its helpers - turns the
draws of one forward into thinned CSRs and noise tensors on the device; `NGCF.propagate` calls it.  Its state lives on the model:
`_filt`, `_filt_maps`, `_row_sorted` and the lazily created `__dict__["_draw_ahead"]`.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import engine as _eng


_HOST_RNG = {"ok": None}


def _host_rng_ok() -> bool:
    """Whether `ngcf_torch_cpu_bernoulli` (csrc/hostrng.hip: torch's CPU `bernoulli_` stream regenerated in vector loops) may stand
    in for torch's own serial kernel in this process: decided once, by drawing 4 099 elements both ways from copies of one
    generator state - flags, kept count and the advanced state must all be equal.  (Another torch build may draw differently - an
    MKL stream, another state layout: then the reference-mode masks keep coming from torch itself, at torch's speed.)"""
    if _HOST_RNG["ok"] is None:
        ok = False
        try:
            import ctypes as C
            lib = _eng._lib.load()
            g = torch.Generator(device="cpu").manual_seed(0x5EED)
            torch.empty(3, dtype=torch.float32).uniform_(generator=g)          # an odd word position
            st = g.get_state().clone()
            n = 4099
            flags = torch.empty(n, dtype=torch.uint8)
            kept = C.c_int64()
            rc = lib.ngcf_torch_cpu_bernoulli(st.data_ptr(), st.numel(), n, 0.7, flags.data_ptr(), None, 0.0, C.byref(kept))
            want = torch.empty(n, dtype=torch.float64).bernoulli_(0.7, generator=g)
            ok = (rc == 0 and torch.equal(flags.bool(), want != 0) and int(kept.value) == int((want != 0).sum())
                  and torch.equal(st, g.get_state()))
        except Exception:  # noqa: BLE001
            ok = False
        _HOST_RNG["ok"] = bool(ok) and os.environ.get("NGCF_HOST_RNG", "1") != "0"
    return _HOST_RNG["ok"]


def _bernoulli_from_state(st: torch.Tensor, n: int, keep: float, noise_shape=None):
    """n draws of Bernoulli(keep) from the mt19937 state bytes `st` (a `torch.get_rng_state()` tensor, advanced in place) through
    `ngcf_torch_cpu_bernoulli`: (keep flags uint8[n] or None, kept count, noise float32 `noise_shape` or None).  Touches neither
    torch's generator nor the GPU (ctypes releases the GIL for the call): safe on a helper thread."""
    import ctypes as C
    flags = None if noise_shape is not None else torch.empty(n, dtype=torch.uint8)
    noise = torch.empty(noise_shape, dtype=torch.float32) if noise_shape is not None else None
    scale = float(torch.ones(1, dtype=torch.float32).div_(keep)) if noise is not None else 0.0
    kept = C.c_int64()
    _eng._lib.check(_eng._lib.load().ngcf_torch_cpu_bernoulli(st.data_ptr(), st.numel(), n, keep, None if flags is None else flags.data_ptr(),
                                                              None if noise is None else noise.data_ptr(), scale, C.byref(kept)))
    return flags, int(kept.value), noise


def _reference_bernoulli(n: int, p_drop: float, noise_shape=None, state: Optional[torch.Tensor] = None):
    """`nn.Dropout(p_drop)` in training mode on a CPU tensor of n ones, drawn from torch's DEFAULT CPU generator exactly as the
    reference draws it (NGCF.py:93-100 on float64 ones, NGCF.py:142 on the float32 activations; both take one 64-bit draw per
    element): returns (keep flags uint8[n] or None, kept count, noise float32 `noise_shape` or None) - the flags for the node
    dropout, the noise tensor (0 or 1/(1-p) as torch rounds it) for the message dropout.  `state`: draw from these state bytes
    (advanced in place) instead of the default generator (`_DrawAhead`; needs `_host_rng_ok()`)."""
    keep = 1.0 - float(p_drop)
    if keep >= 1.0 or keep <= 0.0:        # torch's dropout returns its input (p = 0) or zeros (p = 1) WITHOUT touching the generator
        kept_all = keep >= 1.0
        if noise_shape is not None:
            return None, -1, torch.full(noise_shape, 1.0 if kept_all else 0.0, dtype=torch.float32)
        return torch.full((n,), 1 if kept_all else 0, dtype=torch.uint8), n if kept_all else 0, None
    if state is not None:
        return _bernoulli_from_state(state, n, keep, noise_shape)
    if _host_rng_ok():
        st = torch.get_rng_state()
        out = _bernoulli_from_state(st, n, keep, noise_shape)
        torch.set_rng_state(st)
        return out
    if noise_shape is not None:
        return None, -1, torch.nn.functional.dropout(torch.ones(noise_shape, dtype=torch.float32), p=p_drop, training=True)
    flags = torch.nn.functional.dropout(torch.ones(n, dtype=torch.float64), p=p_drop, training=True).type(torch.bool)
    return flags, int(flags.sum()), None


def _draw_program(program, state: Optional[torch.Tensor] = None):
    """The draws of ONE forward in the reference's order (NGCF.py:123-142), as a generator of (keep flags, kept count, noise) per
    layer.  `program` = (stored entries of L, node-dropout p or None, message-dropout p per layer or None, N, widths): the node
    mask of layer k has one flag per entry the earlier layers kept (cumulative, NGCF.py:126), so the sizes follow from the draws
    themselves - nothing here depends on the batch or on the GPU."""
    nnz, p_node, drops, N, widths = program
    n = nnz
    for k in range(len(widths) - 1):
        flags = kept = noise = None
        if p_node is not None:
            flags, kept, _ = _reference_bernoulli(n, p_node, None, state)
            n = kept
        if drops is not None and drops[k] > 0:
            noise = _reference_bernoulli(N * widths[k + 1], drops[k], (N, widths[k + 1]), state)[2]
        yield flags, kept, noise


class _DrawAhead:
    """r04: the NEXT forward's reference-mode masks, drawn on a helper thread while this step's launches, backward and optimizer run.
    The masks of a forward are a function of the generator state alone (`_draw_program`), so when a forward ends the helper starts
    from a COPY of the state the forward left behind and runs the same program again; the next forward takes the result only if the
    default generator is still in exactly that state (nobody seeded it or drew from it in between) and the program is the same
    (same year slice, same dropout rates, same mode) - it then installs the state the helper ended in, as if it had drawn itself.
    Anything else: the result is dropped and the masks are drawn in place.  Bit-identical either way.  Off: NGCF_DRAW_AHEAD=0."""

    MAX_BYTES = 64 << 20                   # (flags + noise of one forward: 7 MB at the Seoul shape; not for C3-sized masks)

    def __init__(self):
        self.thread, self.job = None, None
        self.hits = self.misses = 0
        # the helper writes into PINNED buffers (two sets, used in turn: the masks of one forward may still be on their way to the
        # device - asynchronous copies out of page-locked memory - while the helper already draws the next ones into the other set)
        self.sets = [{}, {}]                # per set: {"program", "flags", "noise", "event"}
        self.turn = 0
        self.spare = {}                     # (program, set index) -> a set put aside when another program came (year slices alternate)
        self.miss_streak = self.pause = 0   # three misses in a row (batches whose programs do not repeat): no helper for 32 forwards
        self.lease_refs = {}                # year slice -> weak reference to the `_Lease` of the last forward's thinned CSRs (here: a copy of the model starts without)

    def __reduce__(self):                  # copy.deepcopy(model), torch.save(model): a copy starts without a helper
        return (_DrawAhead, ())

    @staticmethod
    def wanted(program) -> bool:
        nnz, p_node, drops, N, widths = program
        size = (3 * nnz if p_node is not None else 0) + (4 * N * sum(widths[1:]) if drops is not None else 0)
        return os.environ.get("NGCF_DRAW_AHEAD", "1") != "0" and size <= _DrawAhead.MAX_BYTES and _host_rng_ok()

    def start(self, program):
        import threading
        if not self.wanted(program):
            self.thread = self.job = None
            return
        import ctypes as C
        # every buffer is allocated HERE and the helper makes ONE foreign call for the whole forward (ngcf_torch_cpu_bernoulli_seq):
        # between two calls it would have to wait for the interpreter lock, which the launching thread gives up every 5 ms at worst
        nnz, p_node, drops, N, widths = program
        node_keep = None if p_node is None else 1.0 - p_node
        if node_keep is not None and not 0.0 < node_keep < 1.0:          # p = 0 / p = 1: torch draws nothing; not worth a helper
            self.thread = self.job = None
            return
        if self.pause > 0:                                               # the programs of this caller's batches do not repeat: stand back
            self.pause -= 1
            self.thread = self.job = None
            return
        self.turn ^= 1
        bset = self.sets[self.turn]
        if bset.get("program") != program:                               # (page-locked allocations are slow: once per program and set)
            if bset.get("program") is not None and len(self.spare) < 6:
                self.spare[(bset["program"], self.turn)] = dict(bset)    # another year slice / mode: its buffers wait for its return
            bset.clear()
            bset.update(self.spare.pop((program, self.turn), {}))
        if bset.get("program") != program:
            pin = torch.cuda.is_available()
            bset.update(program=program, event=None,
                        flags=[torch.empty(nnz, dtype=torch.uint8, pin_memory=pin) for _ in widths[1:]] if node_keep is not None else None,
                        noise=[torch.empty((N, w), dtype=torch.float32, pin_memory=pin) if drops is not None and drops[k] > 0 else None
                               for k, w in enumerate(widths[1:])])
        elif bset["event"] is not None:
            bset["event"].synchronize()                                  # the copies that read this set two forwards ago (long done)
        draws, slots = [], []                # draws: (n or -1, keep, flags, noise, scale) as the C routine takes them; slots: per layer
        for k in range(len(widths) - 1):
            fl = nz = i_fl = None
            if node_keep is not None:
                fl = bset["flags"][k]                                    # (a layer keeps at most what layer 0 started from)
                i_fl = len(draws)
                draws.append((nnz if k == 0 else -1, node_keep, fl, None, 0.0))     # -1: as many as the previous layer kept
            if drops is not None and drops[k] > 0:
                pk = 1.0 - drops[k]
                nz = bset["noise"][k]
                if 0.0 < pk < 1.0:
                    draws.append((N * widths[k + 1], pk, None, nz, float(torch.ones(1, dtype=torch.float32).div_(pk))))
                else:
                    nz.fill_(1.0 if pk >= 1.0 else 0.0)
            slots.append((fl, i_fl, nz))
        m = len(draws)
        job = {"program": program, "start": torch.get_rng_state(), "end": None, "rc": None}
        st = job["start"].clone()
        c_n, c_keep = (C.c_int64 * m)(*[d[0] for d in draws]), (C.c_double * m)(*[d[1] for d in draws])
        c_flags = (C.c_void_p * m)(*[None if d[2] is None else d[2].data_ptr() for d in draws])
        c_noise = (C.c_void_p * m)(*[None if d[3] is None else d[3].data_ptr() for d in draws])
        c_scale, c_kept = (C.c_float * m)(*[d[4] for d in draws]), (C.c_int64 * m)()
        fn = _eng._lib.load().ngcf_torch_cpu_bernoulli_seq
        st_ptr, st_len = st.data_ptr(), st.numel()

        def work():
            job["rc"] = fn(st_ptr, st_len, m, c_n, c_keep, c_flags, c_noise, c_scale, c_kept)     # (the GIL is released for the call)

        def finish():                        # on the taking thread: (flags cut to what was drawn, kept count, noise) per layer
            if job["rc"] != 0:
                return None
            out, n_flags = [], nnz
            for fl, i_fl, nz in slots:
                kept = None
                if fl is not None:
                    fl, kept = fl[:n_flags], int(c_kept[i_fl])
                    n_flags = kept
                out.append((fl, kept, nz))
            job["end"] = st
            return out
        job["finish"] = finish
        self.job = job
        # (not a daemon: the interpreter waits for it at exit - a millisecond at most - instead of freeing the buffers under it)
        self.thread = threading.Thread(target=work, name="ngcf-draw-ahead", daemon=False)
        self.thread.start()

    def copied(self):
        """The forward has queued its copies of the masks it took: the set they live in is free once the stream got past them."""
        bset = self.sets[self.turn]
        if torch.cuda.is_available() and bset.get("program") is not None:
            if bset["event"] is None:
                bset["event"] = torch.cuda.Event()
            bset["event"].record()

    def take(self, program):
        """The helper's masks for `program` if they are the ones this forward would draw now, else None."""
        job, thread = self.job, self.thread
        self.job = self.thread = None
        if job is None:
            return None
        thread.join()
        result = job["finish"]() if job["program"] == program and torch.equal(job["start"], torch.get_rng_state()) else None
        if result is None:
            self.misses += 1
            self.miss_streak += 1
            if self.miss_streak >= 3:
                self.miss_streak, self.pause = 0, 32
            return None
        torch.set_rng_state(job["end"])
        self.hits += 1
        self.miss_streak = 0
        return result


class _Lease:
    """Who may still need the thinned CSRs of ONE forward.  The next forward takes their device buffers over (`filtered(...,
    reuse=...)` moves the handle and leaves the old object empty) - which is only right when the forward they were made for can no
    longer run a backward: its autograd node is gone (the lease is dead: only the CSR lists on the node hold it), or its backward has
    run (`done`).  While a forward still awaits its backward - two forwards before one backward - the next one gets buffers of its
    own.  `recycled`: the buffers WERE handed on after a backward; a second backward through that forward (`retain_graph=True`)
    says so instead of multiplying with another step's matrix."""
    __slots__ = ("done", "recycled", "__weakref__")

    def __init__(self):
        self.done = self.recycled = False


class _LeasedCSRs(list):
    """The per-layer CSRs of one forward (`Propagate` keeps the list for its backward) with the lease of their buffers."""
    lease: Optional[_Lease] = None


def lease_of(csrs) -> Optional[_Lease]:
    return getattr(csrs, "lease", None)


def _take_over_allowed(ahead, year_idx: int):
    """(may this forward recycle the thinned CSRs of the previous reference-mode forward on this year slice?, the lease of its
    own) - see `_Lease`.  The buffers are kept per year slice (`model._filt`), and so are the leases."""
    import weakref
    ref = ahead.lease_refs.get(year_idx)
    prev = ref() if ref is not None else None
    ok = prev is None or prev.done
    if prev is not None and ok:
        prev.recycled = True
    lease = _Lease()
    ahead.lease_refs[year_idx] = weakref.ref(lease)
    return ok, lease


def reference_draws(model, year_idx: int, node_ref: bool, drop, mess_ref: bool):
    """Everything the reference draws from torch's default CPU generator during one forward, in its order
    (NGCF.py:123-142): per layer first the node-dropout keep mask (`nn.Dropout(p)` on float64 ones, on the
    matrix already thinned by the earlier layers: cumulative, unscaled, NGCF.py:93-100), then the message-dropout
    noise tensor (`nn.Dropout(p_k)` on the [N, d_k+1] activations, NGCF.py:142; no draw for p == 0, as in torch).
    Same `torch.manual_seed` -> bit-identical kept edge sets and zero patterns as the reference on CPU.
    Returns (per-layer thinned CSRs or None, their transposes' builder or None, per-layer noise tensors or None).
    """
    dev = model._dev()
    N = model.n_user + model.n_item
    widths = model._widths
    csrs, flags, masks = [], [], []
    if node_ref:
        L = model.lap_list[year_idx]
        row_sorted = model._row_sorted.get(id(L))
        if row_sorted is None:
            r = L._indices()[0]
            row_sorted = model._row_sorted[id(L)] = bool(r.numel() < 2 or not bool((r[1:] < r[:-1]).any()))
        if not row_sorted:           # entry numbers of the stored COO differ from the CSR's: the rebuild path (matrix.py emits sorted rows)
            return _reference_draws_rebuild(model, year_idx, drop, mess_ref)
        src = model.laplacian_csr(year_idx)
    # torch's CPU bernoulli spreads a draw over every thread it may use; on a many-core host (a GPU node's 256 CPUs) that is
    # slower than a few threads by an order of magnitude (26 ms instead of ~3 ms for 0.9 M flags).  The numbers drawn do not
    # depend on the thread count (each chunk skips ahead in one stream), so the draws run on at most 16 threads.
    n_thr = torch.get_num_threads()
    if n_thr > 16:
        torch.set_num_threads(16)
    try:
        return _reference_draws_body(model, year_idx, node_ref, drop, mess_ref, src if node_ref else None, dev, N, widths)
    finally:
        if n_thr > 16:
            torch.set_num_threads(n_thr)


def _reference_draws_body(model, year_idx, node_ref, drop, mess_ref, src, dev, N, widths):
    csrs, flags, masks = _LeasedCSRs(), [], []
    program = (src.nnz if node_ref else 0, float(model.node_dropout) if node_ref else None,
               tuple(float(x) for x in drop) if mess_ref else None, N, tuple(widths))
    ahead = model.__dict__.get("_draw_ahead")
    if ahead is None:
        ahead = model.__dict__["_draw_ahead"] = _DrawAhead()
    draws = ahead.take(program)                          # drawn by the helper thread during the previous step, or None
    take_over = True
    if node_ref:
        take_over, csrs.lease = _take_over_allowed(ahead, year_idx)
    ahead_hit = draws is not None                        # (then the masks sit in page-locked buffers: asynchronous copies)
    for k, (keep, n_kept, noise) in enumerate(draws if ahead_hit else _draw_program(program)):
        if node_ref:
            # one flag per entry of the matrix as the previous layers left it (cumulative, NGCF.py:126); the thinned CSR is a
            # device compaction of the previous one into buffers this module keeps from step to step (ngcf_csr_filter)
            keep = keep.to(dev, non_blocking=ahead_hit)
            src = src.filtered(keep, None, n_kept, reuse=model._filt.pop(("L", year_idx, k), None) if take_over else None)
            model._filt[("L", year_idx, k)] = src
            csrs.append(src)
            flags.append(keep)
        masks.append(noise.to(dev, non_blocking=ahead_hit) if noise is not None else None)
    if ahead_hit:
        ahead.copied()
    ahead.start(program)                                 # the next forward's masks, from the state this one leaves behind
    # the thinned matrices are not symmetric: their transposes are built only if a backward needs them
    return (csrs if node_ref else None, (lambda: _thinned_transposes(model, year_idx, csrs, flags, take_over)) if node_ref else None,
            masks if mess_ref else None)


def _thinned_transposes(model, year_idx: int, csrs, flags, take_over: bool = True):
    """(thinned L_k)^T for every layer, as device compactions of the cached L^T (and of each other): entry j of the transpose
    is kept iff the flag of its twin in L_k-1 is set, found through an entry map that is carried from layer to layer.
    `take_over`: the previous forward's transposes may be recycled (`_Lease`); the returned list shares the lease of `csrs`."""
    dev = model._dev()
    src_t = model.laplacian_csr_t(year_idx)
    emap = model._csr_cache.get(("Tmap", year_idx, id(model.lap_list[year_idx]), str(dev)))
    if emap is None:
        raise RuntimeError("reference-mode node dropout: more than 2^31 stored entries")
    lib = _eng._lib.load()
    out = _LeasedCSRs()
    out.lease = lease_of(csrs)
    for k, (csr_k, keep) in enumerate(zip(csrs, flags)):
        n_src = src_t.nnz
        t = src_t.filtered(keep, emap, csr_k.nnz, reuse=model._filt.pop(("T", year_idx, k), None) if take_over else None)
        model._filt[("T", year_idx, k)] = t
        out.append(t)
        if k + 1 < len(csrs):
            nxt = model._filt_maps.get((year_idx, k))
            if nxt is None or nxt.numel() < max(csr_k.nnz, 1) or nxt.device != dev:
                nxt = model._filt_maps[(year_idx, k)] = torch.empty(max(n_src, 1), dtype=torch.int32, device=dev)
            with _eng._on(dev):
                _eng._lib.check(lib.ngcf_csr_filter_remap(t._h, _eng._ptr(keep), _eng._ptr(emap), n_src,
                                                          _eng.C.c_void_p(csr_k.filter_pos), _eng._ptr(nxt), _eng._stream()))
            emap = nxt[:csr_k.nnz]
        src_t = t
    return out


def _reference_draws_rebuild(model, year_idx: int, drop, mess_ref: bool):
    """The same draws for a `lap_list` entry whose COO is not row-sorted: the mask numbers entries in stored order, so the
    thinned COO is formed with torch indexing and a CSR is built from it per layer (one-off shapes; `Matrix` emits sorted rows)."""
    dev = model._dev()
    N = model.n_user + model.n_item
    widths = model._widths
    csrs, kept, masks = [], [], []
    L = model.lap_list[year_idx]
    idx = L._indices().to(dev)
    val = L._values().to(device=dev, dtype=torch.float32)
    for k in range(model.n_layer):
        mask = _reference_bernoulli(int(val.numel()), model.node_dropout)[0].to(dev).bool()
        idx, val = idx[:, mask], val[mask]
        order = torch.sort(idx[0], stable=True).indices
        csrs.append(_eng.LaplacianCSR.from_coo(idx[0][order], idx[1][order], val[order], N, N))
        kept.append((idx, val))
        if mess_ref and drop[k] > 0:
            masks.append(_reference_bernoulli(N * widths[k + 1], drop[k], (N, widths[k + 1]))[2].to(dev, non_blocking=False))
        else:
            masks.append(None)
    return csrs, (lambda: [model._transposed_csr(i, v)[0] for i, v in kept]), masks if mess_ref else None
