"""Seeded state-machine programs for `NGCF`'s default-on replay and caches, and the twin runner that executes them.

The Python state that decides which kernels run on which buffers - `graphed.forward_graphed` (inference graphs), `train_graphs`
(training graphs), `autograd.E0Cache` (the retained all_E) and the small caches around them - does not fault when it is wrong: it
returns the previous batch's rows, a stale parameter's output, or a held tensor that changed under its holder.  This module draws
long sequences of SUPPORTED calls (`program`), checks on the host that a sequence contains the orderings those caches depend on
(`check_program`: no GPU needed), and runs it on several identically built models that differ only in which of the mechanisms are on
(`Twins`).  Twin against twin everything is compared bit for bit after every action; the eval forwards are anchored to the fp64
oracle so that the twins cannot be wrong together.

Not a conftest and not a test module: tests/test_model_twins_programs.py (CPU) and tests/test_model_state_machine_gpu.py import it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

U, I = 600, 30                                  # the sizes of tests/test_reference_loop_gpu.py
NUM = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
SIZES = (96, 40, 25, 7, 1)
YEARS = (18, 19, 20)
B_CRIT = 96                                     # the constructor batch size of every BPR (the divisor, bprloss.py:22)
ATOL, RTOL = 2e-5, 2e-3                         # tests/test_parity_gpu.py's ATOL, RTOL for all_E against the oracle (copied, not chosen)
TWIN_CONFIGS = ("plain", "default", "cache")

EVAL_OPS = ("eval", "eval25")
TRAIN_VARIANTS = ("plain", "keep_loss", "zero_keep", "accum2", "two_fwd")   # each a full step; see Twins._train
HOLD_WHAT = ("items", "users", "items_slice", "users_slice")
REPLACE_WHAT = ("item", "user", "w1")


@dataclass(frozen=True)
class Action:
    """One call pattern that applies to any twin.  `op` and what `arg` holds:
      eval ()            eval forward under no_grad with negatives, sizes (n, n, n)
      eval25 ()          the 25 users x 25 items x empty neg_item forward of experiment.py:82-91
      propagate ()       model.propagate(year_idx) under no_grad
      train (node_flag, variant)   a full training step, variant of TRAIN_VARIANTS
      fwd_drop (node_flag,)        a forward with grad whose outputs are dropped without a backward
      hold (what, id) / release (id)
      train_mode () / eval_mode () / manual_seed (s,) / snapshot () / load_snapshot ()
      year_new (y,) / year_fill (y,) / size (n,) / modes (node, mess) / emb_ratio (r,)
      to_cpu_and_back () / check_indices () / replace (what, delta)"""
    op: str
    arg: tuple = ()

    def __str__(self):
        return self.op + (repr(self.arg) if self.arg else "")


# ----------------------------------------------------------------------------------------------------------------------------------
# the host-side model of which path a call takes and under which key (graphed._graph_key, train_graphs.forward_train_graphed)
# ----------------------------------------------------------------------------------------------------------------------------------
class _Sim:
    def __init__(self):
        self.size, self.year, self.training = SIZES[0], YEARS[0], True
        self.node_mode = self.mess_mode = "device"
        self.emb_ratio, self.epoch = 1.0, 0      # epoch: bumped where every parameter address changes (`.to()`) or one does (replace)

    def apply(self, a: Action):
        if a.op == "size":
            self.size = a.arg[0]
        elif a.op in ("year_new", "year_fill"):
            self.year = a.arg[0]
        elif a.op == "train_mode":
            self.training = True
        elif a.op == "eval_mode":
            self.training = False
        elif a.op == "modes":
            self.node_mode, self.mess_mode = a.arg
        elif a.op == "emb_ratio":
            self.emb_ratio = a.arg[0]
        elif a.op in ("to_cpu_and_back", "replace"):
            self.epoch += 1

    def inf_key(self, op):
        sizes = (25, 25, 0) if op == "eval25" else (self.size,) * 3
        return ("inf", sizes, self.year, self.emb_ratio, self.epoch)

    def train_key(self, node_flag):
        """None where the forward keeps the eager path whatever happens (`train_graph_wanted`: host-drawn masks)."""
        if (node_flag and self.node_mode != "device") or (self.training and self.mess_mode != "device"):
            return None
        return ("train", (self.size,) * 3, self.year, self.emb_ratio, self.epoch, bool(node_flag), self.node_mode, self.mess_mode, self.training)

    def draws(self, node_flag) -> bool:
        return bool(node_flag) or self.training   # node dropout 0.3 with node_flag; message dropout 0.1 in train mode

    def forwards(self, a: Action) -> list:
        """The keys of the `forward` calls of one action in order (None: an eager call outside both graph paths)."""
        if a.op in EVAL_OPS:
            return [None if self.training else self.inf_key(a.op)]
        if a.op == "train":
            return [self.train_key(a.arg[0])] * (2 if a.arg[1] in ("accum2", "two_fwd") else 1)
        if a.op == "fwd_drop":
            return [self.train_key(a.arg[0])]
        return []


def _project(key):
    """A key without the emb_ratio and the address epoch: what the issue counts as a distinct shape."""
    return key[:3] + key[5:]


def trace(prog: List[Action]):
    """[(action index, key or None)] of every forward call of a program, and per action the simulated state before it."""
    sim, calls = _Sim(), []
    for i, a in enumerate(prog):
        for k in sim.forwards(a):
            calls.append((i, k))
        sim.apply(a)
    return calls


def expected_training_replays(prog: List[Action]) -> int:
    """A lower bound of `_train_calls` on the default twin (calls answered by the training graphs, the capturing one included) in
    device-mode terms: every call of a key after its first, less every call that has a documented reason to run eagerly - a
    forward inside a hold (the held tensor may be a replay's static result), the second forward of `two_fwd` (the first still
    awaits its backward) and one forward per `manual_seed` (the first drawing forward after it re-seeds in place)."""
    calls = [(i, k) for i, k in trace(prog) if k is not None and k[0] == "train"]
    per_key = {}
    for _, k in calls:
        per_key[k] = per_key.get(k, 0) + 1
    spans, opened = [], {}
    for i, a in enumerate(prog):
        if a.op == "hold":
            opened[a.arg[1]] = i
        elif a.op == "release":
            spans.append((opened.pop(a.arg[0]), i))
    in_hold = sum(any(h < i < r for h, r in spans) for i, _ in calls)
    two_fwd = sum(a.op == "train" and a.arg[1] == "two_fwd" for a in prog)
    reseeds = sum(a.op == "manual_seed" for a in prog)
    return max(0, sum(n - 1 for n in per_key.values()) - in_hold - two_fwd - reseeds)


def check_program(prog: List[Action], kind: str) -> Dict[str, int]:
    """The orderings a program was built for, asserted on the host.  `kind`: "inference" (no optimizer), "training" (one dropout mode,
    read as device mode - the reference-mode program is the same text) or "mixed".  Returns the figures it checked.

    "In a row" for a training key means: a run of training-path forwards of that key that no training-path forward of another key
    interrupts (an eval forward or a `manual_seed` in between leaves the captured graphs where they are)."""
    calls = trace(prog)
    stats = {}
    has_train = kind != "inference"
    # every hold is released, ids are unique
    open_holds = {}
    spans = []
    for i, a in enumerate(prog):
        if a.op == "hold":
            assert a.arg[1] not in open_holds
            open_holds[a.arg[1]] = i
        elif a.op == "release":
            spans.append((open_holds.pop(a.arg[0]), i))
    assert not open_holds, "a hold is never released"
    inf_calls = [(i, k) for i, k in calls if k is not None and k[0] == "inf"]
    tr_calls = [(i, k) for i, k in calls if k is not None and k[0] == "train"]
    stats["inference_keys"] = len({_project(k) for _, k in inf_calls})
    stats["training_keys"] = len({_project(k) for _, k in tr_calls})
    assert stats["inference_keys"] >= 10, stats
    if has_train:
        assert stats["training_keys"] >= 6, stats
        # every training key recurs at least 3 times in a row somewhere (eager, capture + replay, replay)
        best, run, last = {}, 0, None
        for _, k in tr_calls:
            run = run + 1 if k == last else 1
            last = k
            best[k] = max(best.get(k, 0), run)
        short = [k for k, n in best.items() if n < 3]
        assert not short, f"training keys that never come 3 times in a row: {short}"
        stats["shortest_training_run"] = min(best.values())
        # a manual_seed between two replays of one training key that draws masks
        seen, hit = {}, 0
        for j, (i, k) in enumerate(tr_calls):
            if j + 1 < len(tr_calls) and seen.get(k, 0) >= 2 and tr_calls[j + 1][1] == k and (k[5] or k[8]):
                hit += any(prog[x].op == "manual_seed" for x in range(i + 1, tr_calls[j + 1][0]))
            seen[k] = seen.get(k, 0) + 1
        stats["reseeds_between_replays"] = hit
        assert hit >= 1, "no manual_seed between two replays of one training key"
    else:
        assert not tr_calls and not any(a.op in ("train", "fwd_drop", "train_mode") for a in prog)
        # each replaced parameter: changed values, followed directly by eval forwards of an already-captured shape
        done = set()
        sim, seen = _Sim(), {}
        for i, a in enumerate(prog):
            if a.op == "replace":
                assert a.arg[1] != 0.0
                nxt = prog[i + 1:i + 3]
                assert len(nxt) == 2 and all(x.op in EVAL_OPS for x in nxt), f"action {i}: a replacement is not followed by eval forwards"
                assert not sim.training and seen.get(sim.inf_key(nxt[0].op), 0) >= 3, \
                    f"action {i}: the shape after the replacement was not captured before it"
                done.add(a.arg[0])
            for k in sim.forwards(a):
                if k is not None:
                    seen[k] = seen.get(k, 0) + 1
            sim.apply(a)
        assert done == set(REPLACE_WHAT), done
    # a hold that spans a replay of the same key: taken right after the >= 3rd call of a key, another call of it before the release
    counts, at = {}, {}
    for n, (i, k) in enumerate(calls):
        if k is not None:
            counts[k] = counts.get(k, 0) + 1
        at[n] = counts.get(k, 0)
    span_hits = {"inf": 0, "train": 0}
    for h, r in spans:
        before = [n for n, (i, _) in enumerate(calls) if i < h]
        if not before:
            continue
        k = calls[before[-1]][1]
        if k is not None and at[before[-1]] >= 3 and any(h < i < r and kk == k for i, kk in calls):
            span_hits[k[0]] += 1
    stats["holds_over_inference_replay"], stats["holds_over_training_replay"] = span_hits["inf"], span_hits["train"]
    assert span_hits["inf"] >= 1, "no hold spans an inference replay of the same key"
    if has_train:
        assert span_hits["train"] >= 1, "no hold spans a training replay of the same key"
    # a run of more than 8 eval forwards with nothing else in between (MAX_TOUCHED overflows), and 17+ consecutive calls of one key
    sim, run, best_run, krun, best_krun, last = _Sim(), 0, 0, 0, 0, None
    for a in prog:
        k = sim.forwards(a)[0] if a.op in EVAL_OPS else None
        if k is not None:
            run += 1
            krun = krun + 1 if k == last else 1
            last = k
        else:
            run, krun, last = 0, 0, None
        best_run, best_krun = max(best_run, run), max(best_krun, krun)
        sim.apply(a)
    stats["longest_eval_run"], stats["longest_one_key_run"] = best_run, best_krun
    assert best_run > 8 and best_krun >= 17, stats
    # both eviction limits: a key comes back after enough OTHER keys to have pushed its graph out (8 inference, 4 training)
    for name, some, limit in (("inference", inf_calls, 8), ("training", tr_calls, 4)):
        back, order, n_calls = 0, [], {}
        for _, k in some:
            if k in order:                                 # (`order`: most recently used last, like the modules' graph tables)
                later = [o for o in order[order.index(k) + 1:] if n_calls[o] >= 2]       # keys that held a graph after k's last use
                back += n_calls[k] >= 2 and len(later) >= limit
                order.remove(k)
            order.append(k)
            n_calls[k] = n_calls.get(k, 0) + 1
        stats[name + "_recaptures_after_eviction"] = back
        assert back >= 1 or (name == "training" and not has_train), f"no {name} key returns after {limit} others"
    return stats


# ----------------------------------------------------------------------------------------------------------------------------------
# program generator
# ----------------------------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, rng, kind, weights):
        self.rng, self.kind, self.w = rng, kind, weights
        self.acts: List[Action] = []
        self.sim = _Sim()
        self.calls: Dict[tuple, int] = {}
        self.hold_id = self.n_variant = 0
        self.has_snapshot = False

    def add(self, op, *arg):
        a = Action(op, tuple(arg))
        for k in self.sim.forwards(a):
            if k is not None:
                self.calls[k] = self.calls.get(k, 0) + 1
        self.acts.append(a)
        self.sim.apply(a)

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def context(self, size=None, year=None):
        if size is not None and size != self.sim.size:
            self.add("size", size)
        if year is not None and year != self.sim.year:
            self.add(self.pick(("year_new", "year_fill")), year)

    def evals(self, n, op=None):
        for _ in range(n):
            self.add(op or self.pick(EVAL_OPS))

    def captured(self, op):
        """Eval forwards of `op` until its key has been called three times (eager, capture + replay, replay)."""
        while self.calls.get(self.sim.inf_key(op), 0) < 3:
            self.add(op)

    def hold(self):
        self.hold_id += 1
        self.add("hold", HOLD_WHAT[self.hold_id % len(HOLD_WHAT)], self.hold_id)          # every kind of hold in turn
        return self.hold_id

    def small(self, op=None):
        """One action that changes no key: what may stand between two calls of a run."""
        op = op or self.pick(("check_indices", "manual_seed", "snapshot", "propagate"))
        if op == "manual_seed":
            self.add(op, int(self.rng.integers(1, 1000)))
        else:
            self.add(op)
            self.has_snapshot |= op == "snapshot"

    def train_run(self, n, node_flag, variants=TRAIN_VARIANTS, extras=True):
        """n training steps of ONE key (>= 3: eager, capture + replay, replay) with key-preserving actions in between."""
        for j in range(n):
            v = "plain"
            if j >= 2:                                     # the variants in turn: none is left to luck
                self.n_variant += 1
                v = variants[self.n_variant % len(variants)]
            if extras and j >= 2 and self.rng.random() < 0.15:
                self.add("fwd_drop", node_flag)
            self.add("train", node_flag, v)
            if extras and j >= 1 and self.rng.random() < 0.2:
                self.add(self.pick(("check_indices", "snapshot")))
                self.has_snapshot |= self.acts[-1].op == "snapshot"

    def node_flag(self):
        """node_flag of the next training run.  In the single-mode training programs every eval-mode step asks for node dropout, as the
        reference's loop does (experiment.py:45): the reference-mode twin of the program then never reaches a capturable forward."""
        if self.kind == "training" and not self.sim.training:
            return True
        return bool(self.rng.random() < 0.6)


def _weighted(rng, weights: Dict[str, float]) -> str:
    names = sorted(weights)
    p = np.array([weights[n] for n in names], dtype=np.float64)
    return names[int(rng.choice(len(names), p=p / p.sum()))]


DEFAULT_WEIGHTS = {
    "inference": {"context": 5, "hold": 2, "small": 2, "load": 1, "to": 0.7, "ratio": 1, "replace": 1.5},
    "training": {"train": 5, "evals": 3, "hold_train": 1, "hold_eval": 1, "small": 1.5, "load": 0.7, "to": 0.5, "ratio": 0.7},
    "mixed": {"train": 5, "evals": 3, "hold_train": 1, "hold_eval": 1, "small": 1.5, "load": 0.7, "to": 0.5, "ratio": 1, "modes": 1.5,
              "flip": 1},
}


def program(seed: int, n_actions: int, kind: str, weights: Optional[Dict[str, float]] = None) -> List[Action]:
    """A sequence of about `n_actions` actions for `kind` ("inference", "training", "mixed"), drawn with
    `numpy.random.default_rng(seed)`.  The orderings the caches depend on are put in by construction (scripted segments, every
    training run at least three steps of one key, the random segments walking through the size x year combinations before they
    repeat one) and verified afterwards: `check_program` runs on every program returned."""
    rng = np.random.default_rng(seed)
    b = _Builder(rng, kind, dict(DEFAULT_WEIGHTS[kind], **(weights or {})))
    combos = [(s, y) for s in SIZES for y in YEARS]
    rng.shuffle(combos)
    turn = [0]

    def next_combo():
        turn[0] += 1
        return combos[turn[0] % len(combos)]

    def replace(what):
        op = b.pick(EVAL_OPS)
        b.captured(op)
        b.add("replace", what, float(b.pick((0.25, -0.125, 0.5))))
        b.evals(2, op)

    def hold_over_evals():
        op = b.pick(EVAL_OPS)
        b.captured(op)
        b.add(op)                                          # (the attributes are this key's replayed result when the hold is taken)
        h = b.hold()
        b.evals(int(rng.integers(1, 4)), op)
        b.add("release", h)

    def hold_over_train(node_flag):
        fresh = b.sim.train_key(node_flag) is None or b.calls.get(b.sim.train_key(node_flag), 0) < 3
        b.train_run(3 if fresh else 1, node_flag, variants=("plain",), extras=False)
        h = b.hold()
        b.train_run(2, node_flag, variants=("plain", "keep_loss"), extras=False)
        b.add("release", h)

    def filler(stop):
        while len(b.acts) < stop:
            seg = _weighted(rng, b.w)
            if seg == "context":
                b.context(*next_combo())
                b.evals(3, b.pick(EVAL_OPS))
            elif seg == "evals":
                if b.sim.training:
                    continue
                if rng.random() < 0.5:
                    b.context(*next_combo())
                b.evals(3, b.pick(EVAL_OPS))
            elif seg == "train":
                b.context(*next_combo())
                b.train_run(int(rng.integers(3, 6)), b.node_flag())
            elif seg == "hold":
                hold_over_evals()
            elif seg == "hold_eval":
                if not b.sim.training:
                    hold_over_evals()
            elif seg == "hold_train":
                hold_over_train(b.node_flag())
            elif seg == "small":
                b.small()
            elif seg == "load":
                if b.has_snapshot:
                    b.add("load_snapshot")
            elif seg == "to":
                b.add("to_cpu_and_back")
            elif seg == "ratio":
                b.add("emb_ratio", 0.5 if b.sim.emb_ratio == 1.0 else 1.0)
            elif seg == "replace":
                replace(b.pick(REPLACE_WHAT))
            elif seg == "modes":
                b.add("modes", b.pick(("device", "reference")), b.pick(("device", "reference")))
            elif seg == "flip":
                b.add("eval_mode" if b.sim.training else "train_mode")

    if kind == "inference":
        b.add("eval_mode")
        b.context(25, 18)
        first = (b.sim.size, b.sim.year)
        b.evals(18, "eval25")                              # > 8 touched batches, > 16 calls of one key
        for what in REPLACE_WHAT:
            replace(what)
        hold_over_evals()
        b.add("snapshot")
        b.has_snapshot = True
        b.context(*first)
        b.evals(3, "eval25")
        for s, y in combos[:10]:                           # ten further shapes: the first graph is evicted
            b.context(s, y)
            b.evals(3, "eval")
        b.context(*first)
        b.evals(3, "eval25")                               # ... and captured again
        b.add("emb_ratio", 0.5)
        b.evals(3, "eval25")
        b.add("load_snapshot")
        b.add("to_cpu_and_back")
        b.evals(3, "eval25")
        b.add("emb_ratio", 1.0)
        for op in ("propagate", "check_indices", "manual_seed"):
            b.small(op)
        for _ in range(3):                                 # with the one above: every kind of hold
            hold_over_evals()
        filler(n_actions)
    else:
        b.add("manual_seed", 12)
        if kind == "mixed":
            # what only this program has at its start: a capturable forward that draws NO masks (eval mode, node_flag False) comes
            # before the first forward that draws - the device seed state does not exist yet when these graphs are captured
            b.add("eval_mode")
            b.context(40, 19)
            b.train_run(3, False, extras=False)
        b.add("train_mode")
        b.context(96, 18)
        first_nf = True
        b.train_run(3, first_nf, extras=False)             # eager, capture, replay
        b.add("train", first_nf, "two_fwd")                # node masks: two forwards, backward through the first only
        b.add("manual_seed", 99)                           # a re-seed between two replays
        b.train_run(2, first_nf, variants=("plain",), extras=False)
        hold_over_train(first_nf)
        b.context(40, 18)
        b.train_run(3, False)                              # train mode, no node dropout: message masks only
        b.add("train", False, "two_fwd")                   # (the same key: two forwards, backward through the first only)
        b.add("eval_mode")                                 # experiment.py:72 - the single-mode programs never call train() again
        b.context(25, 18)
        b.evals(18, "eval25")                              # > 8 touched batches, > 16 calls of one key
        hold_over_evals()
        b.context(96, 18)
        b.train_run(3, first_nf)                           # the eval-mode key of the first shape ...
        b.add("train", first_nf, "two_fwd")
        for (s, y), nf in zip([c for c in combos if c != (96, 18)][:5], (True, True, kind == "training", True, kind == "training")):
            b.context(s, y)
            b.train_run(3, nf)                             # ... five further keys: more than 4 pairs of graphs
        b.context(96, 18)
        b.train_run(3, first_nf)                           # ... and it is captured again
        b.context(25, 18)
        b.evals(3, "eval25")
        for s, y in combos[5:14]:                          # nine further inference shapes: more than 8 graphs
            b.context(s, y)
            b.evals(3, "eval")
        b.context(25, 18)
        b.evals(3, "eval25")
        b.add("snapshot")
        b.has_snapshot = True
        for op in ("propagate", "check_indices"):
            b.small(op)
        b.add("emb_ratio", 0.5)
        b.context(7, 20)
        b.train_run(4, True)
        b.add("fwd_drop", True)
        b.evals(3, "eval")
        b.add("load_snapshot")
        b.add("emb_ratio", 1.0)
        b.add("to_cpu_and_back")
        b.train_run(3, True)
        hold_over_train(True)                              # with the two above and the next: every kind of hold
        hold_over_evals()
        filler(n_actions)
        if kind == "mixed":
            # both dropout modes and train() after eval(), whatever the random segments drew
            b.add("eval_mode")
            b.add("modes", "reference", "device")
            b.context(40, 20)
            b.train_run(3, True)                           # host-drawn node masks: eager
            b.add("train_mode")
            b.add("modes", "device", "device")
            b.train_run(3, True)
            b.add("eval_mode")
    # every open hold is closed by construction; a last eval forward so that the final state is looked at once more
    if not b.sim.training:
        b.evals(1)
    check_program(b.acts, kind)
    return b.acts


# the four programs of tests/test_model_state_machine_gpu.py (and of the host-side check in tests/test_model_twins_programs.py)
PROGRAMS = {
    "inference_65": dict(seed=101, n_actions=200, kind="inference", embed=65, layers=(65, 65), modes=("device", "device")),
    "inference_60": dict(seed=102, n_actions=200, kind="inference", embed=60, layers=(64, 64), modes=("device", "device")),
    "training_device": dict(seed=103, n_actions=200, kind="training", embed=65, layers=(65, 65), modes=("device", "device")),
    "training_reference": dict(seed=103, n_actions=200, kind="training", embed=65, layers=(65, 65), modes=("reference", "reference")),
    "mixed": dict(seed=104, n_actions=200, kind="mixed", embed=60, layers=(64, 64), modes=("device", "device")),
}


def program_of(name: str) -> List[Action]:
    spec = PROGRAMS[name]
    return program(spec["seed"], spec["n_actions"], spec["kind"])


# ----------------------------------------------------------------------------------------------------------------------------------
# the twins and the runner
# ----------------------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _bits_equal(a, b) -> bool:
    """Bit for bit; None only equals None.  Keeps no reference to either tensor."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    if a.is_floating_point():
        return bool(torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32)))
    return bool(torch.equal(a, b))


def _attr_equal(ma, mb, name) -> bool:
    """`model.all_users_emb` / `all_items_emb` of two twins, through temporaries only: the modules read reference counts, and this
    harness must not count as a holder."""
    return _bits_equal(getattr(ma, name), getattr(mb, name))


class _Twin:
    def __init__(self, name, model, opt, crit, test_crit):
        self.name, self.model, self.opt, self.crit, self.test_crit = name, model, opt, crit, test_crit
        self.total_loss = 0                                # experiment.py:59 `total_loss += loss`
        self.kept: List[Tuple[torch.Tensor, torch.Tensor]] = []     # (held tensor, its clone at hold time): losses
        self.held: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.snapshot = None


class Twins:
    """N models of the package's NGCF from one `torch.manual_seed`, on the same `lap_list`, in identical initial state:
      plain    auto_graph = auto_train_graph = reuse_all_E = False - the path the parity and backward tests pin to the oracle
      default  everything as constructed: all three on
      cache    graphs off, reuse_all_E on: the retained all_E carries every eval forward
    each with its own `optim.Adam` (unless `with_optimizer=False`) and its own BPR criteria."""

    def __init__(self, pkg, dev, lap, embed, layers, modes=("device", "device"), with_optimizer=True, seed=4, configs=TWIN_CONFIGS):
        self.pkg, self.dev, self.lap = pkg, dev, lap
        self.twins: List[_Twin] = []
        for name in configs:
            torch.manual_seed(seed)
            m = pkg.NGCF(embed, list(layers), 0.3, [0.1] * len(layers), 1.0, lap, NUM, B_CRIT, dev).to(dev)
            if name == "plain":
                m.auto_graph = m.auto_train_graph = m.reuse_all_E = False
            elif name == "cache":
                m.auto_graph = m.auto_train_graph = False
            else:
                assert m.auto_graph and m.auto_train_graph and m.reuse_all_E
            m.node_dropout_mode, m.mess_dropout_mode = modes
            opt = pkg.optim.Adam(m.parameters(), lr=1e-2) if with_optimizer else None
            self.twins.append(_Twin(name, m, opt, pkg.BPR(0.025, B_CRIT), pkg.BPR(0.025, 25)))
        sd0 = self.twins[0].model.state_dict()
        for t in self.twins[1:]:
            sd = t.model.state_dict()
            assert list(sd) == list(sd0) and all(_bits_equal(sd[k], sd0[k]) for k in sd0), "the twins do not start equal"
        self.default = next((t.model for t in self.twins if t.name == "default"), None)
        self.size, self.year_val = SIZES[0], YEARS[0]
        self.year: Dict[int, torch.Tensor] = {}
        self.anchors = 0
        self.last_anchor = -10 ** 9
        self.coo = {}

    # ---- batches ----------------------------------------------------------------------------------------------------------------
    def _year_tensor(self, n):
        if n not in self.year:
            self.year[n] = torch.full((n,), self.year_val, device=self.dev)
        return self.year[n]

    def _batch(self, g, n, with_neg=True):
        r = lambda hi: torch.randint(0, hi, (n,), generator=g).to(self.dev)  # noqa: E731
        b = dict(year=self._year_tensor(n), u_id=r(U), age=r(76), sex=r(2), month=r(13), day=r(32), dow=r(7), pos_item=r(I), neg_item=r(I))
        k = min(5, n // 2)
        if k:
            b["u_id"][:k] = b["u_id"][k:2 * k]             # duplicates in every batch, as tests/test_reference_loop_gpu.py forces them
        if not with_neg:
            b["neg_item"] = torch.empty(0)
        return b

    def _batches(self, a: Action, g):
        if a.op == "eval":
            return [self._batch(g, self.size)]
        if a.op == "eval25":
            return [self._batch(g, 25, with_neg=False)]
        if a.op == "train":
            return [self._batch(g, self.size) for _ in range(2 if a.arg[1] in ("accum2", "two_fwd") else 1)]
        if a.op == "fwd_drop":
            return [self._batch(g, self.size)]
        return []

    # ---- one action on one twin ------------------------------------------------------------------------------------------------------
    def _eval(self, t: _Twin, a: Action, batch):
        m = t.model
        with torch.no_grad():
            u, p, n = m(node_flag=False, **batch)
            if a.op == "eval":
                loss = t.crit(u, p, n)
            else:
                loss = t.test_crit(u, p[:1], torch.cat((p[1:], p[1:][:1])))       # experiment.py:96-101
        out = {"u": u, "p": p, "n": n, "loss": loss}
        if not m.training:
            # block 0 of all_E IS cat(user table, item table) after the injection, bit for bit (NGCF.py:120)
            d0 = m.emb_size
            if not (torch.equal(m.all_users_emb[:, :d0], m.user_embedding.weight.detach()) and
                    torch.equal(m.all_items_emb[:, :d0], m.item_embedding.weight.detach())):
                out["error"] = "block 0 of all_E is not the embedding tables"
        return out

    def _train(self, t: _Twin, a: Action, batches):
        m, opt, crit = t.model, t.opt, t.crit
        node_flag, variant = a.arg
        out = {}
        if variant == "accum2":                            # two backward passes accumulated before one step()
            u, p, n = m(node_flag=node_flag, **batches[0])
            opt.zero_grad()
            first = crit(u, p, n)
            first.backward()
            u, p, n = m(node_flag=node_flag, **batches[1])
            loss = crit(u, p, n)
            loss.backward()
            out["first_loss"] = first.detach()
        elif variant == "two_fwd":                         # two forwards, backward through the first only
            u, p, n = m(node_flag=node_flag, **batches[0])
            u2, p2, n2 = m(node_flag=node_flag, **batches[1])
            out["u2"], out["p2"], out["n2"] = u2.detach(), p2.detach(), n2.detach()
            del u2, p2, n2
            opt.zero_grad()
            loss = crit(u, p, n)
            loss.backward()
        else:
            u, p, n = m(node_flag=node_flag, **batches[0])
            opt.zero_grad(set_to_none=(variant != "zero_keep"))
            loss = crit(u, p, n)
            loss.backward()
        opt.step()
        if variant == "keep_loss":
            t.total_loss = t.total_loss + loss             # every step's autograd graph stays referenced (experiment.py:59)
            t.kept.append((loss, loss.detach().clone()))
        out.update(u=u.detach(), p=p.detach(), n=n.detach(), loss=loss.detach())
        return out

    def _held_tensor(self, m, what):
        if what == "items":
            return m.all_items_emb
        if what == "users":
            return m.all_users_emb
        if what == "items_slice":
            return m.all_items_emb[3:9]
        return m.all_users_emb[:5]

    def _replace(self, m, what, delta):
        mod = {"item": m.item_embedding, "user": m.user_embedding, "w1": m.w1_list[len(m.w1_list) - 1]}[what]
        mod.weight = torch.nn.Parameter(mod.weight.detach() + delta)

    def _apply(self, t: _Twin, a: Action, batches):
        m = t.model
        if a.op in EVAL_OPS:
            return self._eval(t, a, batches[0])
        if a.op == "train":
            return self._train(t, a, batches)
        if a.op == "fwd_drop":
            u, p, n = m(node_flag=a.arg[0], **batches[0])
            return {"u": u.detach(), "p": p.detach(), "n": n.detach()}
        if a.op == "propagate":
            with torch.no_grad():
                m.propagate(self.year_val % 18)
        elif a.op == "hold":
            if m.all_items_emb is None or m.all_users_emb is None:
                return {"error": "nothing to hold: the model has no all_*_emb"}
            h = self._held_tensor(m, a.arg[0])
            t.held[a.arg[1]] = (h, h.detach().clone())
        elif a.op == "release":
            if a.arg[0] not in t.held:
                return {"error": "this twin never took the hold that is released"}
            h, c = t.held.pop(a.arg[0])
            if not _bits_equal(h, c):
                return {"error": "a held tensor changed under its holder"}
        elif a.op == "train_mode":
            m.train()
        elif a.op == "eval_mode":
            m.eval()
        elif a.op == "manual_seed":
            torch.manual_seed(a.arg[0])
        elif a.op == "snapshot":
            t.snapshot = {k: v.detach().clone() for k, v in m.state_dict().items()}
        elif a.op == "load_snapshot":
            m.load_state_dict(t.snapshot)
        elif a.op == "modes":
            m.node_dropout_mode, m.mess_dropout_mode = a.arg
        elif a.op == "emb_ratio":
            m.emb_ratio = a.arg[0]
        elif a.op == "to_cpu_and_back":
            m.to("cpu")
            m.to(self.dev)
        elif a.op == "check_indices":
            m.check_indices_now()
        elif a.op == "replace":
            self._replace(m, *a.arg)
        elif a.op in ("size", "year_new", "year_fill"):
            pass                                           # (the runner's own state: `_shared`)
        else:
            raise ValueError(a.op)
        return {}

    def _shared(self, a: Action):
        """What an action changes in the runner itself, once (not per twin)."""
        if a.op == "size":
            self.size = a.arg[0]
        elif a.op == "year_new":
            self.year_val, self.year = a.arg[0], {}                     # new tensor objects from now on
        elif a.op == "year_fill":
            self.year_val = a.arg[0]
            for y in self.year.values():
                y.fill_(a.arg[0])                                       # the same objects: `_version` moves

    # ---- the fp64 anchor ---------------------------------------------------------------------------------------------------------
    def _anchor(self):
        import ngcf_oracle as orc
        m = self.twins[0].model
        assert self.twins[0].name == "plain"
        yi = self.year_val % 18
        if yi not in self.coo:
            L = self.lap[yi].cpu()
            self.coo[yi] = (L._indices()[0].numpy(), L._indices()[1].numpy(), L._values().numpy())
        sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        E0 = np.concatenate([sd["user_embedding.weight"], sd["item_embedding.weight"]])
        n = m.n_layer
        want = orc.propagate_f64(*self.coo[yi], E0, [sd[f"w1_list.{k}.weight"] for k in range(n)], [sd[f"w1_list.{k}.bias"] for k in range(n)],
                                 [sd[f"w2_list.{k}.weight"] for k in range(n)], [sd[f"w2_list.{k}.bias"] for k in range(n)])
        got = torch.cat((m.all_users_emb, m.all_items_emb), 0).detach().cpu().numpy()
        self.anchors += 1
        bad = np.abs(got - want) > ATOL + RTOL * np.abs(want)
        if bad.any():
            return f"all_E of `plain` is off the fp64 oracle at {int(bad.sum())} elements, max abs error {float(np.abs(got - want).max()):.3e}"
        return None

    # ---- the run -----------------------------------------------------------------------------------------------------------------
    def _fail(self, prog, i, what):
        lines = [f"action {i}: {prog[i]}: {what}", "the 10 actions before it:"]
        lines += [f"  {j}: {prog[j]}" for j in range(max(0, i - 10), i)]
        raise Mismatch("\n".join(lines))

    def _compare(self, prog, i, results, states):
        """Twin against twin after one action, bit for bit.  Every reference to a result dies with this frame."""
        names = [t.name for t in self.twins]
        ref = self.twins[0]
        for t, res, st in zip(self.twins, results, states):
            if "error" in res:
                self._fail(prog, i, f"twin `{t.name}`: {res['error']}")
            if not torch.equal(st, states[0]):
                self._fail(prog, i, f"the default CPU generator ends in another state on `{t.name}` than on `{names[0]}`")
            if set(res) != set(results[0]):
                self._fail(prog, i, f"`{t.name}` returned {sorted(res)}, `{names[0]}` {sorted(results[0])}")
            for k in res:
                if not _bits_equal(res[k], results[0][k]):
                    self._fail(prog, i, f"`{k}` of `{t.name}` differs from `{names[0]}`")
            if t is ref:
                continue
            for name in ("all_users_emb", "all_items_emb"):
                if not _attr_equal(t.model, ref.model, name):
                    self._fail(prog, i, f"model.{name} of `{t.name}` differs from `{names[0]}`")
            pa, pb = dict(ref.model.named_parameters()), dict(t.model.named_parameters())
            for k in pa:
                if not _bits_equal(pa[k], pb[k]):
                    self._fail(prog, i, f"parameter {k} of `{t.name}` differs from `{names[0]}`")
                if not _bits_equal(pa[k].grad, pb[k].grad):
                    self._fail(prog, i, f"the gradient of {k} on `{t.name}` differs from `{names[0]}`")
            del pa, pb

    def run(self, prog: List[Action], batch_seed: int = 31, anchor_every_eval: bool = False, progress=None):
        g = torch.Generator().manual_seed(batch_seed)
        for i, a in enumerate(prog):
            self._shared(a)
            batches = self._batches(a, g)
            before = torch.get_rng_state()
            results, states = [], []
            for t in self.twins:
                torch.set_rng_state(before)                # the twins never see each other's draws
                try:
                    results.append(self._apply(t, a, batches))
                except Mismatch:
                    raise
                except Exception as e:  # noqa: BLE001
                    self._fail(prog, i, f"twin `{t.name}` raised {type(e).__name__}: {e}")
                states.append(torch.get_rng_state())
            torch.set_rng_state(states[0])
            self._compare(prog, i, results, states)             # (in a frame of its own: nothing of it outlives the call)
            del results
            if a.op in EVAL_OPS and not self.twins[0].model.training and (anchor_every_eval or i - self.last_anchor >= 25):
                self.last_anchor = i
                err = self._anchor()
                if err:
                    self._fail(prog, i, err)
            if progress is not None:
                progress(i, a)
        # copy-on-hold at the end: the losses kept in the `total_loss` chain are what they were
        for t in self.twins:
            for n_, (h, c) in enumerate(t.kept):
                if not _bits_equal(h, c):
                    raise Mismatch(f"kept loss {n_} of twin `{t.name}` changed under its holder")
            assert not t.held, "a program left a hold open"
            if t.kept and not _bits_equal(t.total_loss.detach(), self.twins[0].total_loss.detach()):
                raise Mismatch(f"total_loss of `{t.name}` differs")

    def bookkeeping(self, kind: str, train_modes=("device", "device"), prog: Optional[List[Action]] = None):
        """The default twin at the end of a program: bounded graph tables, and it really left the eager path."""
        m = self.default
        assert len(m._graphs) <= 8 and len(m._train_graphs) <= 4, (len(m._graphs), len(m._train_graphs))
        assert len(m._graphs) >= 1 and m._graph_calls >= 1, "the default twin never replayed an inference graph"
        if kind == "inference":
            assert m._train_calls == 0 and not m._train_graphs
        elif "reference" in train_modes and kind == "training":
            assert m._train_calls == 0 and not m._train_graphs, "host-drawn masks: nothing to capture, and nothing captured"
        else:
            assert len(m._train_graphs) >= 1 and m._train_calls >= 1, "the default twin never replayed a training graph"
            if prog is not None:
                want = expected_training_replays(prog)
                assert want >= 20 and m._train_calls >= want, f"{m._train_calls} training replays, the program has at least {want}"
        return {"graphs": len(m._graphs), "graph_calls": m._graph_calls, "train_graphs": len(m._train_graphs),
                "train_calls": m._train_calls, "anchors": self.anchors}
