"""The CU-free exchange of include/ngcf_hip.h (`ngcf_p2p_*`) and the row collectives built on it.  Every user follows one protocol:
`fence()` before pulls into memory that queued kernels may still use, a `pull_from_all` round, `join()` before the next reader."""

import ctypes as C
import os

import torch
import torch.distributed as dist

from .. import _lib, engine as _eng


def sum_slots(slots: torch.Tensor, out: torch.Tensor):
    """out = slots[0] + slots[1] + ... in slot order (ngcf_sum_slots_f32): the owner's side of a reduce-scatter done with pulls."""
    n = out.numel()
    assert slots.is_contiguous() and out.is_contiguous() and slots.numel() == slots.shape[0] * n
    with _eng._on(out.device):
        _lib.check(_lib.load().ngcf_sum_slots_f32(_eng._ptr(slots), n, slots.shape[0], n, _eng._ptr(out), _eng._stream()))


class P2PExchange:
    """The CU-free exchange of include/ngcf_hip.h (`ngcf_p2p_*`): one exchange buffer per rank, peers pull from it with
    device-to-device copies on copy-engine streams, host threads do the waiting.  All ranks of `group` must live on one node
    (IPC handles + POSIX shared memory).  `floats(offset, n)` gives a tensor over this rank's buffer: producers write there."""

    TIMEOUT_MS = float(os.environ.get("NGCF_P2P_TIMEOUT_MS", "60000"))

    def __init__(self, group, device, n_floats: int):
        lib = _lib.load()
        self.group, self.dev = group, torch.device(device)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.n_floats = int(n_floats)
        tok = [os.urandom(8).hex() if self.rank == 0 else None]
        dist.broadcast_object_list(tok, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        self.name = f"ngcf_p2p_{tok[0]}"
        # Every rank takes part in every collective of this constructor whatever happened to it locally (a rank that raised
        # between two of them would leave the others waiting in the next one): failures travel with the gathered objects and
        # all ranks raise together.
        h, err = C.c_void_p(), None
        mine = (C.c_char * 64)()
        try:
            with _eng._on(self.dev):
                _lib.check(lib.ngcf_p2p_create(self.rank, self.world, max(self.n_floats, 64) * 4, self.name.encode(), C.byref(h)))
            _lib.check(lib.ngcf_p2p_handle(h, mine))
        except Exception as exc:  # noqa: BLE001
            err = f"rank {self.rank}: {exc!r}"[:300]
        self._h = h
        got = [None] * self.world
        dist.all_gather_object(got, (err, bytes(mine.raw)), group=group)
        errs = [e for e, _ in got if e]
        if not errs:
            try:
                blob = (C.c_char * (64 * self.world)).from_buffer_copy(b"".join(hb for _, hb in got))
                with _eng._on(self.dev):
                    _lib.check(lib.ngcf_p2p_connect(self._h, blob))
            except Exception as exc:  # noqa: BLE001
                err = f"rank {self.rank}: {exc!r}"[:300]
            got2 = [None] * self.world
            dist.all_gather_object(got2, err, group=group)      # (doubles as the barrier: everyone is connected before the first pull)
            errs = [e for e in got2 if e]
        if errs:
            self.close_quietly()
            raise RuntimeError("p2p exchange could not be set up: " + "; ".join(errs))
        self.base = int(lib.ngcf_p2p_local(self._h))
        self._mem = _eng._device_view(self.base, max(self.n_floats, 64), torch.float32, self.dev)   # the exchange buffer
        assert self._mem.data_ptr() == self.base and self._mem.dtype == torch.float32
        self.seq = {}                      # slot -> last published / expected step

    def floats(self, offset: int, n: int) -> torch.Tensor:
        assert 0 <= offset and offset + n <= self.n_floats
        return self._mem[offset:offset + n]

    def publish(self, slot: int, seq: int):
        _lib.check(_lib.load().ngcf_p2p_publish(self._h, slot, seq, _eng._stream()))

    def pull(self, peer: int, slot: int, seq: int, src_off_floats: int, dst: torch.Tensor):
        """dst (contiguous, this device) <- rank `peer`'s exchange buffer [src_off, src_off + dst.numel()), once it published `seq`."""
        assert dst.is_contiguous() and dst.dtype == torch.float32
        _lib.check(_lib.load().ngcf_p2p_pull(self._h, peer, slot, seq, src_off_floats * 4, C.c_void_p(dst.data_ptr()),
                                             dst.numel() * 4, self.TIMEOUT_MS))

    def ack(self, peer: int, slot: int, seq: int):
        _lib.check(_lib.load().ngcf_p2p_ack(self._h, peer, slot, seq))

    def wait_acks(self, slot: int, seq: int):
        _lib.check(_lib.load().ngcf_p2p_wait_acks(self._h, slot, seq, self.TIMEOUT_MS))

    def fence(self):
        _lib.check(_lib.load().ngcf_p2p_fence(self._h, _eng._stream()))

    def join(self):
        _lib.check(_lib.load().ngcf_p2p_join(self._h, _eng._stream()))

    def stats(self, reset: bool = False):
        """(host milliseconds spent blocked in waits, waits, waits that found their word missing) since creation / the last reset."""
        ms, n, nb = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().ngcf_p2p_stats(self._h, C.byref(ms), C.byref(n), C.byref(nb), 1 if reset else 0))
        return float(ms.value), int(n.value), int(nb.value)

    def peers_from(self, start: int):
        """All ranks, beginning after `start` (every rank starts its pulls at another peer: the links are used evenly)."""
        return [(start + 1 + q) % self.world for q in range(self.world)]

    def pull_from_all(self, slot: int, seq: int, src_off_floats: int, dst_of, ack=None):
        """One pull round: `dst_of(q)` <- every rank q's exchange buffer at `src_off_floats` (this rank's own included), once q
        published `seq` on `slot`.  `ack` = (slot, seq): each peer is told so right after its pull is enqueued - it may then
        overwrite what was read; None where the reader acknowledges later (several rounds read one pass's buffer)."""
        for q in self.peers_from(self.rank):
            self.pull(q, slot, seq, src_off_floats, dst_of(q))
            if ack is not None:
                self.ack(q, *ack)

    def selftest(self) -> bool:
        """Every rank writes a pattern, publishes it, pulls every peer's and compares; True on every rank iff it worked everywhere."""
        ok = 1
        try:
            n = 1024
            probe = self.floats(0, n)
            probe.copy_(torch.arange(n, dtype=torch.float32, device=self.dev) + 1000.0 * self.rank)
            self.publish(63, 1)
            got = torch.empty((self.world, n), dtype=torch.float32, device=self.dev)
            # `got` may reuse the block of a temporary whose kernels are still queued on this stream (the allocator hands memory
            # out by stream order): the copies must not land before them.  (Without this fence the self-test failed one run in
            # three with five ranks on one GPU: a pending kernel of the old owner wrote over the pulled rows.)
            self.fence()
            self.pull_from_all(63, 1, 0, lambda q: got[q], ack=(63, 1))
            self.join()
            torch.cuda.synchronize(self.dev)
            want = torch.arange(n, dtype=torch.float32, device=self.dev)[None] + 1000.0 * torch.arange(self.world, device=self.dev)[:, None]
            ok = int(torch.equal(got, want))
            self.wait_acks(63, 1)
        except Exception as exc:  # noqa: BLE001
            ok = 0
            self.last_error = f"rank {self.rank}: {exc!r}"[:300]
        if ok == 0 and not getattr(self, "last_error", None):
            self.last_error = f"rank {self.rank}: pulled rows differ from what the peers wrote"
        errs = [None] * self.world                       # every rank learns what failed where (the bench line quotes it)
        dist.all_gather_object(errs, getattr(self, "last_error", None) if ok == 0 else None, group=self.group)
        errs = [e for e in errs if e]
        if errs:
            self.last_error = "; ".join(errs)[:600]
        return not errs

    def close_quietly(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.load().ngcf_p2p_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:  # noqa: BLE001
            pass

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.dev)
            self._mem = None
            _lib.load().ngcf_p2p_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class P2PCollectives:
    """All-gather and reduce-scatter of row blocks over a `P2PExchange` of its own: the exchange steps of the TRAINING path (forward
    and backward) without a collective kernel on the CUs.  Every call uses the next of four regions of the exchange buffer and its
    sequence slot in turn (all ranks issue the same sequence of calls), so a producer overwrites a region only after every peer has
    read what it held four calls earlier.  The host blocks in each call until the peers have published (no pipelining here)."""

    REGIONS = 4

    def __init__(self, group, device, region_floats: int):
        self.region = int(region_floats)
        self.ex = P2PExchange(group, device, self.REGIONS * self.region)
        self.rank, self.world, self.dev = self.ex.rank, self.ex.world, self.ex.dev
        self._op, self._last = 0, {}

    def _stage(self, t: torch.Tensor):
        """The rows of `t` [n, d] into the next region of this rank's exchange buffer (row stride d4 = d rounded up to 4 floats:
        every rank's block is then a whole number of 16-byte pieces), published; returns (slot, seq, region offset, d4)."""
        n, d = t.shape
        d4 = (d + 3) // 4 * 4
        assert t.dtype == torch.float32 and n * d4 <= self.region, "P2PCollectives: block larger than a region"
        reg = self._op % self.REGIONS
        self._op += 1
        slot, seq, off = 32 + reg, self._op, reg * self.region
        self.ex.wait_acks(slot, self._last.get(slot, 0))
        self.ex.floats(off, n * d4).view(n, d4)[:, :d].copy_(t)
        self.ex.publish(slot, seq)
        self._last[slot] = seq
        self.ex.fence()                          # the copies below land in fresh tensors: after whatever used that memory before
        return slot, seq, off, d4

    def all_gather(self, send: torch.Tensor) -> torch.Tensor:
        m, d = send.shape
        slot, seq, off, d4 = self._stage(send)
        full = torch.empty((self.world * m, d4), dtype=torch.float32, device=self.dev)
        self.ex.pull_from_all(slot, seq, off, lambda q: full[q * m:(q + 1) * m], ack=(slot, seq))
        self.ex.join()
        return full[:, :d]

    def reduce_scatter(self, full: torch.Tensor) -> torch.Tensor:
        m, d = full.shape[0] // self.world, full.shape[1]
        slot, seq, off, d4 = self._stage(full)
        slots = torch.empty((self.world, m, d4), dtype=torch.float32, device=self.dev)
        self.ex.pull_from_all(slot, seq, off + self.rank * m * d4, lambda q: slots[q], ack=(slot, seq))
        self.ex.join()
        own = torch.empty((m, d4), dtype=torch.float32, device=self.dev)
        sum_slots(slots, own)
        return own[:, :d]                        # (the padding columns carry whatever the regions held: never read)
