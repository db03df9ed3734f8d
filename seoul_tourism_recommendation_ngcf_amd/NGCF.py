"""`NGCF` - the reference's nn.Module surface, backed by the HIP propagation engine.

Drop-in for `/root/reference/model/NGCF.py:7-156`: same constructor, same keyword `forward`,
same parameter names/shapes (so the reference's 23 checkpoints load with `strict=True`), same
externally read attributes (`all_users_emb`, `all_items_emb`, demo.py:233), same in-place
mutation of `user_embedding.weight` (NGCF.py:114-115).  What differs is where the work runs:
every tensor op of the forward body is a hand-written gfx950 kernel behind the C ABI in
`include/ngcf_hip.h`; torch only owns the memory.  There is no CPU path: calling `forward`
with the module on the CPU raises.

This file holds the module itself: constructor, buffers, CSR caches, seed state, `propagate` and `forward`.  What `forward`
and `propagate` hand over to lives beside it: the reference-mode mask draws in `reference_masks`, the auto-captured
inference forward in `graphed` (`forward_graphed`), the auto-captured training forward in `train_graphs`.  All three keep
their state on the model.  The two graph modules import this one, so `forward` imports them when it first needs them.
"""
from __future__ import annotations

import os
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from . import engine as _eng
from .autograd import E0Cache, GatherTriple, propagate_with_grad
from .reference_masks import reference_draws


def _spmm_mode() -> int:
    """SpMM kernel choice for the cached Laplacians (include/ngcf_hip.h, ngcf_csr_set_mode); NGCF_SPMM_MODE overrides."""
    return int(os.environ.get("NGCF_SPMM_MODE", "3"))


def _raise_bad_index(status: torch.Tensor, mirror: Optional[torch.Tensor]):
    """Read a (sticky) status word - one host sync; if a kernel saw an out-of-range id, clear the word and its pinned host mirror
    (which only ever holds a copy of it) and raise."""
    if int(status.item()) != 0:
        status.zero_()
        if mirror is not None:
            mirror.zero_()
        raise IndexError("index out of range in NGCF.forward (u_id / feature ids / pos_item / neg_item)")


class NGCF(nn.Module):
    def __init__(self,
                 embed_size: int,
                 layer_size: list,
                 node_dropout: float,
                 mess_dropout: list,
                 emb_ratio: float,
                 lap_list: list,
                 num_dict: dict,
                 batch_size: int,
                 device):
        super().__init__()
        self.n_user = num_dict['user']
        self.n_item = num_dict['item']
        self.emb_size = embed_size
        self.weight_size = layer_size
        self.n_layer = len(self.weight_size)
        self.batch_size = batch_size
        self.device = device
        self.node_dropout = node_dropout
        self.mess_dropout = mess_dropout
        self.emb_ratio = emb_ratio

        # registration order fixes the state_dict key order of the reference's checkpoints
        fw = self.emb_size // 5                                     # NGCF.py:39-43
        self.month_emb = nn.Embedding(num_dict['month'], fw)
        self.day_emb = nn.Embedding(num_dict['day'], fw)
        self.sex_emb = nn.Embedding(num_dict['sex'], fw)
        self.age_emb = nn.Embedding(num_dict['age'], fw)
        self.dow_emb = nn.Embedding(num_dict['dayofweek'], fw)
        self.item_embedding = nn.Embedding(self.n_item, self.emb_size)
        self.user_embedding = nn.Embedding(self.n_user, self.emb_size)

        self.lap_list = lap_list                                    # borrowed, NGCF.py:52
        for emb in (self.user_embedding, self.item_embedding, self.age_emb, self.sex_emb,
                    self.month_emb, self.dow_emb, self.day_emb):    # NGCF.py:58-68
            nn.init.kaiming_uniform_(emb.weight)

        # W1_k then W2_k per layer, as set_layers does (NGCF.py:73-78): the same torch.manual_seed then gives the same
        # initial Linear weights as the reference class (tests/test_reference_checkpoints.py)
        dims = self._widths
        w1, w2 = [], []
        for k in range(self.n_layer):
            w1.append(nn.Linear(dims[k], dims[k + 1], bias=True))
            w2.append(nn.Linear(dims[k], dims[k + 1], bias=True))
        self.w1_list = nn.Sequential(*w1)
        self.w2_list = nn.Sequential(*w2)
        self.node_dropout_list = nn.Sequential(
            *[nn.Dropout(p=self.node_dropout) for _ in range(self.n_layer if self.node_dropout is not None else 0)])
        self.mess_dropout_list = nn.Sequential(
            *[nn.Dropout(p=self.mess_dropout[k]) for k in range(self.n_layer if self.mess_dropout is not None else 0)])

        # engine state (not part of the state_dict)
        self._csr_cache = {}
        self._filt = {}                  # thinned CSRs of the reference-mode node dropout, re-used from step to step
        self._filt_maps = {}             # entry maps of their transposes
        self._row_sorted = {}            # id(lap_list entry) -> its COO rows are non-decreasing
        self._ws = _eng.Workspace()
        self._carry: List[Optional[torch.Tensor]] = [None, None]
        self._scratch: Optional[torch.Tensor] = None
        self._status: Optional[torch.Tensor] = None
        self._status_host: Optional[torch.Tensor] = None
        self.check_indices = True        # raise IndexError on out-of-range ids (one host sync per forward)
        # where the random masks come from: "reference" = torch's default CPU generator, drawn exactly where the reference
        # draws (bit-identical masks for the same torch.manual_seed, one host round trip per layer); "device" = counter
        # hash evaluated inside the kernels (same distribution and semantics, another stream, no host work)
        self.node_dropout_mode = "reference"
        self.mess_dropout_mode = "reference"
        self.all_users_emb = None
        self.all_items_emb = None
        self._all_E = None
        # Inference calls (eval mode, no autograd, node_flag=False) of launch-bound sizes are captured into a hipGraph on first
        # use and replayed afterwards (`graphed.forward_graphed`): unchanged callers (experiment.py:66-119, demo.py:213-236) get the
        # replay speed without knowing about it.  `auto_graph = False` switches it off.
        self.auto_graph = True
        self.auto_graph_max_bytes = 64 << 20     # all_E above this size: the forward is not launch-bound, nothing to gain
        self.index_check_every = 16              # graph replays: read the (sticky) status word every k-th call; 1 = every call
        self._graphs = {}                        # (sizes, year slice, parameter addresses) -> GraphedForward, most recent last
        self._graph_calls = 0
        self._graph_seen = set()
        self._plist = None
        self._year_tag, self._year_idx = None, 0
        self._forced_year_idx = None
        # Training calls (train mode, autograd on) of launch-bound sizes with both dropouts drawn on the DEVICE: forward and backward
        # are captured as two hipGraphs on the second call of a shape (`train_graphs._TrainGraphs`, over the eager path) and
        # replayed afterwards; `loss.backward()` then replays the backward graph.  Unchanged training loops (experiment.py:45-58) get
        # a host cost of two graph launches for the model's share of the step.  `auto_train_graph = False` switches it off.
        self.auto_train_graph = True
        self._alias = None                       # (capture only) the parameter aliases propagate() differentiates instead of the parameters
        self._train_graphs = {}                  # key -> graphed core module, most recent last
        self._train_seen = {}                    # key -> the stream its first (eager) call ran on
        self._train_calls = 0
        self._capture_warned = False
        # Inference forwards keep their all_E and skip the copy of E0 into block 0 while both embedding tables are unchanged and
        # nobody else holds the previous result (autograd.E0Cache).  `reuse_all_E = False`: a fresh all_E and a full copy per call.
        self.reuse_all_E = True
        self._e0_cache = E0Cache()

    # ------------------------------------------------------------------------------------
    # engine plumbing
    # ------------------------------------------------------------------------------------
    def _dev(self) -> torch.device:
        dev = self.user_embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError(
                "NGCF propagation engine: parameters are on '%s'. This module runs hand-written HIP kernels for "
                "MI355X only and has no CPU fallback; call .to('cuda') first." % dev)
        return dev

    @property
    def _widths(self) -> list:
        """Column widths of all_E's blocks: E0, then one per layer."""
        return [self.emb_size] + list(self.weight_size)

    def _all_E_bytes(self) -> int:
        return (self.n_user + self.n_item) * sum(self._widths) * 4

    def _mess_drop(self) -> List[float]:
        """The message-dropout rate of every layer as this forward applies it: nn.Dropout follows train()/eval(), NGCF.py:142."""
        if self.training and self.mess_dropout is not None:
            return [float(p) for p in self.mess_dropout[:self.n_layer]]
        return [0.0] * self.n_layer

    def _status_buf(self, dev):
        if self._status is None or self._status.device != dev:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._status

    def _status_host_buf(self):
        """Pinned host mirror of `_status`: the captured training forward copies the word there as its last node (r04), so
        `_peek_status` sees an earlier replay's out-of-range id without a host sync."""
        if self._status_host is None:
            self._status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        return self._status_host

    def _peek_status(self):
        """Raise IndexError for an out-of-range id of any graph replay the GPU has finished - no host sync unless there is one."""
        h = self._status_host
        if h is not None and int(h[0]) != 0:
            self.check_indices_now()
        for g in list(self._graphs.values()):
            g.peek_status()

    def _raise_if_status(self):
        """IndexError if the module's own status word is set (a host sync).  The inference graphs have a word each: `check_status`."""
        _raise_bad_index(self._status, self._status_host)

    def _scratch_buf(self, dev):
        if self._scratch is None or self._scratch.device != dev or self._scratch.numel() != self.n_user:
            self._scratch = torch.full((self.n_user,), -1, dtype=torch.int32, device=dev)
        return self._scratch

    def _feature_tables(self):
        return (self.age_emb.weight.data, self.sex_emb.weight.data, self.month_emb.weight.data, self.day_emb.weight.data,
                self.dow_emb.weight.data)

    def _inject_features(self, features, u_idx: torch.Tensor, status: torch.Tensor):
        """NGCF.py:103-115 for all of `u_idx` at once: `features` = (age, sex, month, day, dow) into `user_embedding.weight.data`, no
        autograd.  A `.data` write: the retained all_E is told which rows to follow (`E0Cache.touch`), here and nowhere else.
        Returns `engine.feature_inject`'s keep-alive (the converted index tensors), held by the caller as long as it sees fit."""
        with torch.no_grad():
            keep = _eng.feature_inject(self.user_embedding.weight.data, self._feature_tables(), features, u_idx, self.emb_ratio,
                                       self._scratch_buf(self._dev()), status)
            self._e0_cache.touch(u_idx)
        return keep

    def laplacian_csr(self, year_idx: int) -> "_eng.LaplacianCSR":
        """CSR of `lap_list[year_idx]`, built once and cached (replaces the per-call `.to(device)`, NGCF.py:118)."""
        dev = self._dev()
        L = self.lap_list[year_idx]            # IndexError for a bad year_idx, like the reference
        key = (year_idx, id(L), str(dev))
        csr = self._csr_cache.get(key)
        if csr is None:
            N = self.n_user + self.n_item
            if tuple(L.shape) != (N, N):
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(L.shape)} and {N}x{self.emb_size})")
            rows, cols, vals = self._sorted_coo(L, dev)
            csr = _eng.LaplacianCSR.from_coo(rows, cols, vals, N, N)
            csr.set_mode(_spmm_mode())         # long-lived matrix: worth the L2-swept plan where that pays
            self._csr_cache = {k: v for k, v in self._csr_cache.items() if year_idx not in k[:2]}
            self._csr_cache[key] = csr
        return csr

    @staticmethod
    def _sorted_coo(L: torch.Tensor, dev):
        """COO triplets of a `lap_list` entry on the device, row-sorted (stable) so that the CSR keeps their order:
        the position of an entry in this order is its entry number (used by the device-side node dropout)."""
        if not L.is_sparse:
            raise RuntimeError("lap_list entries must be torch sparse COO tensors (matrix.py:79-83)")
        idx = L._indices().to(dev)
        val = L._values().to(device=dev, dtype=torch.float32)
        rows, cols = idx[0], idx[1]
        if rows.numel() > 1 and bool((rows[1:] < rows[:-1]).any()):
            order = torch.sort(rows, stable=True).indices
            rows, cols, val = rows[order], cols[order], val[order]
        return rows, cols, val

    def laplacian_csr_t(self, year_idx: int) -> "_eng.LaplacianCSR":
        """CSR of `lap_list[year_idx]` transposed (for `L^T . dLE` in the backward), built on first use."""
        dev = self._dev()
        L = self.lap_list[year_idx]
        key = ("T", year_idx, id(L), str(dev))
        csr = self._csr_cache.get(key)
        if csr is None:
            rows, cols, vals = self._sorted_coo(L, dev)
            csr, order = self._transposed_csr(torch.stack([rows, cols]), vals)
            csr.set_mode(_spmm_mode())
            self._csr_cache[key] = csr
            # entry j of L^T is entry order[j] of L: lets the reference-mode node dropout thin L^T with the flags drawn for L
            self._csr_cache[("Tmap",) + key[1:]] = order.to(torch.int32) if order.numel() < 2 ** 31 - 1 else None
        return csr

    def _transposed_csr(self, idx: torch.Tensor, val: torch.Tensor):
        """CSR of the transpose (the device-mode edge dropout is keyed by (row, column) of L: no entry map is needed) and the
        position in L of every entry of L^T."""
        N = self.n_user + self.n_item
        order = torch.sort(idx[1], stable=True).indices          # by column = row of L^T, original order kept inside
        return _eng.LaplacianCSR.from_coo(idx[1][order], idx[0][order], val[order], N, N), order

    def _diff_params(self):
        """The parameters a training forward differentiates, in the order `_alias` is read: the two embedding tables, then W1, b1,
        W2, b2 of every layer (the feature tables enter through `.data`, NGCF.py:103-115: no gradient)."""
        w1, b1, w2, b2 = self._layer_params()
        return [self.user_embedding.weight, self.item_embedding.weight, *w1, *b1, *w2, *b2]

    def _layer_params(self):
        return ([l.weight for l in self.w1_list], [l.bias for l in self.w1_list],
                [l.weight for l in self.w2_list], [l.bias for l in self.w2_list])

    def _private_seeds(self, n: int):
        """64-bit seeds for the device-mode hash streams, from a generator of the module's own: the default CPU stream is
        consumed only where the reference consumes it.  Follows torch.manual_seed (re-seeded when the default seed changes)."""
        src = torch.initial_seed()
        if getattr(self, "_seed_gen", None) is None or self._seed_src != src:
            self._seed_gen = torch.Generator(device="cpu").manual_seed(src ^ 0x5DEECE66D)
            self._seed_src = src
        return [int(x) for x in torch.randint(0, 2 ** 62, (n,), dtype=torch.int64, generator=self._seed_gen)]

    def _device_seeds(self) -> torch.Tensor:
        """The 2 n_layer seed words of ONE training forward, as a fresh device tensor.  A persistent state tensor is seeded from
        the module's private generator (which follows `torch.manual_seed`: the first forward after seeding uses exactly the values
        `_private_seeds` would hand out) and stepped on the device before every later forward (`ngcf_seeds_advance`); the forward
        gets a copy of its own, so a backward that runs after another forward still recomputes its own masks.  No host random
        numbers, no host round trip - and inside a captured hipGraph every replay draws new masks."""
        dev = self._dev()
        n = 2 * self.n_layer
        src = torch.initial_seed()
        st = getattr(self, "_seed_state", None)
        if st is None or st.device != dev or st.numel() != n or self._seed_state_src != src:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("device-mode dropout: run one training forward before capturing (the seed state is created on first use)")
            fresh = torch.tensor(self._private_seeds(n), dtype=torch.int64, device=dev)
            if st is not None and st.device == dev and st.numel() == n:
                st.copy_(fresh)                  # re-seeded (torch.manual_seed): in place - captured graphs bake this tensor's address in
            else:
                self._seed_state = fresh
            self._seed_state_src = src
        else:
            with _eng._on(dev):                  # (the launch stream must be the MODEL's device's, whatever device is current)
                _eng._lib.check(_eng._lib.load().ngcf_seeds_advance(_eng._ptr(self._seed_state), n, _eng._stream()))
        return self._seed_state.clone()

    # ------------------------------------------------------------------------------------
    # propagation (NGCF.py:120-149)
    # ------------------------------------------------------------------------------------
    def propagate(self, year_idx: int = 0, node_flag: bool = False) -> torch.Tensor:
        """all_E = [E0 | norm(E1) | ... | norm(En)]  for the current parameters; sets all_users_emb/all_items_emb."""
        self._dev()
        if self.node_dropout_mode not in ("reference", "device"):
            raise ValueError("node_dropout_mode must be 'reference' or 'device'")
        if self.mess_dropout_mode not in ("reference", "device"):
            raise ValueError("mess_dropout_mode must be 'reference' or 'device'")
        drop = self._mess_drop()
        node_ref = bool(node_flag) and self.node_dropout_mode == "reference"
        mess_ref = any(p > 0 for p in drop) and self.mess_dropout_mode == "reference"
        csrs, csrs_t_fn, masks = None, None, None
        if node_ref or mess_ref:
            csrs, csrs_t_fn, masks = reference_draws(self, year_idx, node_ref, drop, mess_ref)
        edge_drops = None
        node_dev = bool(node_flag) and csrs is None                    # node dropout in "device" mode: the cached CSR, thinned in-kernel
        if csrs is None:
            csrs = [self.laplacian_csr(year_idx)] * self.n_layer
            csrs_t_fn = lambda: [self.laplacian_csr_t(year_idx)] * self.n_layer   # noqa: E731
        mess_dev = any(p > 0 for p in drop) and masks is None
        seeds = [0] * self.n_layer
        keep_alive = None
        if node_dev or mess_dev:
            # "device" modes: the seeds of this forward live in device memory and reach the kernels as tagged addresses
            # (include/ngcf_hip.h, NGCF_SEED_PTR_TAG): words 0..n-1 the node-dropout seeds (layer k uses 0..k: cumulative, unscaled -
            # the mask is a counter-based hash of (seed, row, column) evaluated inside the SpMM), words n..2n-1 the message-dropout
            # seeds of the layer epilogues.  The backward recomputes the masks from the same words.
            keep_alive = self._device_seeds()
            tag = lambda i: (0xD5ED << 48) | (keep_alive.data_ptr() + 8 * i)   # noqa: E731
            if node_dev:
                ns = [tag(k) for k in range(self.n_layer)]
                edge_drops = [(ns[:k + 1], float(self.node_dropout)) for k in range(self.n_layer)]
            if mess_dev:
                seeds = [tag(self.n_layer + k) for k in range(self.n_layer)]
        w1, b1, w2, b2 = self._layer_params()
        uw, iw = self.user_embedding.weight, self.item_embedding.weight
        if self._alias is not None:                                    # _TrainGraphs: same storage, fresh autograd leaves
            n = self.n_layer
            uw, iw = self._alias[0], self._alias[1]
            w1, b1, w2, b2 = (self._alias[2 + j * n:2 + (j + 1) * n] for j in range(4))
        all_E = propagate_with_grad(self, csrs, csrs_t_fn, uw, iw, w1, b1, w2, b2, drop, seeds, edge_drops, masks, keep_alive)
        self._all_E = all_E
        self.all_users_emb = all_E[:self.n_user, :]                    # NGCF.py:148-149
        self.all_items_emb = all_E[self.n_user:, :]
        return all_E

    # ------------------------------------------------------------------------------------
    # forward (NGCF.py:102-156)
    # ------------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        self._plist = None
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._plist = None
        self._train_graphs.clear()               # (their static buffers live on the old device / dtype)
        self._e0_cache.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def invalidate_all_E(self):
        """Forget the retained all_E (`reuse_all_E`): the next inference forward copies E0 in full.  Needed only after a write to an
        embedding table through `.data` from outside this module (such writes bypass the version counter the cache watches)."""
        self._e0_cache.invalidate()

    def load_state_dict(self, *args, **kwargs):
        self._plist = None
        return super().load_state_dict(*args, **kwargs)

    def _year_index(self, year: torch.Tensor) -> int:
        """`year.unique()[0] % 18` (NGCF.py:117) = the smallest year of the batch, read back from the device once per tensor:
        the same tensor OBJECT passed again unmodified (same version counter) needs no second host sync."""
        if self._forced_year_idx is not None:          # GraphedTrainStep: the slice was fixed when the step was captured
            return self._forced_year_idx
        if not year.numel():
            return 0
        ref, ver = self._year_tag if self._year_tag is not None else (None, -1)
        if ref is None or ref() is not year or ver != year._version:    # identity of the OBJECT (an address alone is re-used by the allocator)
            self._year_idx = int(year.min().item() % 18)
            self._year_tag = (weakref.ref(year), year._version)
        return self._year_idx

    def check_indices_now(self):
        """Raise IndexError if any graph-replayed forward since the last check saw an out-of-range id."""
        for g in self._graphs.values():
            g.check_status()
        if self._train_graphs and self._status is not None:
            self._raise_if_status()

    def forward(self, year, u_id, age, sex, month, day, dow, pos_item, neg_item, node_flag):
        dev = self._dev()
        status = self._status_buf(dev)
        fw = self.emb_size // 5
        if 5 * fw != self.emb_size:
            # the reference fails at NGCF.py:114 with a shape-mismatch RuntimeError for such widths
            raise RuntimeError(f"shape mismatch: value tensor of shape [{len(u_id)}, {5 * fw}] cannot be broadcast "
                               f"to indexing result of shape [{len(u_id)}, {self.emb_size}]")
        if (self.auto_graph and not self.training and not node_flag and not torch.is_grad_enabled() and len(u_id) > 0 and
                len(pos_item) > 0 and self._all_E_bytes() <= self.auto_graph_max_bytes
                and not torch.cuda.is_current_stream_capturing()):
            from .graphed import forward_graphed
            out = forward_graphed(self, dev, year, u_id, age, sex, month, day, dow, pos_item, neg_item)
            if out is not None:
                return out
        from .train_graphs import forward_train_graphed, train_graph_wanted
        if train_graph_wanted(self, node_flag, u_id, pos_item, neg_item):
            out = forward_train_graphed(self, dev, year, u_id, age, sex, month, day, dow, pos_item, neg_item, node_flag)
            if out is not None:
                return out
        # feature injection into user_embedding.weight.data, no autograd (NGCF.py:103-115)
        u_idx = u_id.to(device=dev, dtype=torch.int64).contiguous()
        keep = self._inject_features((age, sex, month, day, dow), u_idx, status)

        year_idx = self._year_index(year)                              # == year.unique()[0] % 18, NGCF.py:117
        self.propagate(year_idx, bool(node_flag))

        p_idx = pos_item.to(device=dev, dtype=torch.int64).contiguous()
        n_idx = neg_item.to(device=dev, dtype=torch.int64).contiguous() if len(neg_item) > 0 else None
        neg_i_embeddings = torch.empty(0)                                       # NGCF.py:153
        if self._all_E.requires_grad:
            outs = GatherTriple.apply(self._all_E, self.n_user, status, u_idx, p_idx, n_idx)
            u_embeddings, pos_i_embeddings = outs[0], outs[1]
            if n_idx is not None:
                neg_i_embeddings = outs[2]
        else:
            u_embeddings, pos_i_embeddings, neg = _eng.gather_rows3(                       # NGCF.py:151-155, one launch
                self._all_E, ((u_idx, 0, self.n_user), (p_idx, self.n_user, self.n_item), (n_idx, self.n_user, self.n_item)), status)
            if neg is not None:
                neg_i_embeddings = neg
        if self.check_indices and not torch.cuda.is_current_stream_capturing():   # (a captured step checks the sticky word after its replay)
            self._raise_if_status()
        del keep
        return u_embeddings, pos_i_embeddings, neg_i_embeddings
