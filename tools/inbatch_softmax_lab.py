"""The softmax loss with shared (in-batch) negatives (InBatchSoftmax: csrc/inbatch_softmax.hip) against two yardsticks, loss plus
backward on the same batch:

- the same loss written in torch ops (`mm` with TF32 off, boolean masks, `logsumexp`, autograd), whose [B, B + E] score matrix and
  the gradient of the same size are in memory;
- `SampledSoftmax` at m = 64 negatives per row, the project's other sampled loss, which gathers B (m + 2) rows where the in-batch
  loss gathers 2 B + E.

Every side starts from the same user and item tables and the batch's ids: the row gathers (torch indexing of the detached tables)
are inside the timed region, the gathered rows are the leaves whose gradients are computed.  Shapes: C3-sized rows (B = 8 192,
D = 512, 100 000 items; E = 0 and E = 1 024) and the Seoul rows (B = 512, D = 260, 100 items, E = 0): ids with the duplicates such a
catalogue gives, corrections as `sampling.item_logq` makes them.  Time, peak device memory on top of the tables, and for the fused
side the achieved share of the fp32-MFMA peak (157.3 TFLOP/s), taking 5 x 2 B (B + E) D flops for forward plus backward.  All sides in
one process, alternating, two warm-ups each, device events around each call; medians of --reps runs.  Writes its lines to --out
(default profiles/inbatch_softmax_lab.txt) as well as to stdout."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

WD, TAU, PEAK, M = 0.025, 1.0, 157.3e12, 64

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_softmax_lab.txt"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


def compare(sides):
    """{name: callable} -> {name: (median ms, min, max, peak bytes, last result)}, alternating after two warm-ups each."""
    for _ in range(2):
        for fn in sides.values():
            measure(fn)
    t = {k: [] for k in sides}
    peak = {k: 0 for k in sides}
    last = {}
    for _ in range(args.reps):
        for k, fn in sides.items():
            ms, pk, last[k] = measure(fn)
            t[k].append(ms)
            peak[k] = max(peak[k], pk)
    return {k: (float(np.median(t[k])), min(t[k]), max(t[k]), peak[k], last[k]) for k in sides}


def torch_ops_loss(u, p, x, ids, xids, lq, xlq, bs):
    B, E = u.shape[0], x.shape[0]
    eye = torch.eye(B, B + E, dtype=torch.bool, device=u.device)
    s = torch.mm(u, torch.cat((p, x)).t()) * (1.0 / TAU)
    s = torch.where(eye, s - lq[:, None], s - torch.cat((lq, xlq))[None, :])
    s = s.masked_fill((torch.cat((ids, xids))[None, :] == ids[:, None]) & ~eye, float("-inf"))
    return ((torch.logsumexp(s, 1) - s.diagonal()).sum() + WD * (u.pow(2).sum() + p.pow(2).sum())) / bs


def lab(B, E, D, n_items, what):
    say(f"Loss + backward, {what}: B = {B}, E = {E}, D = {D}, {n_items} items, random rows (scores around +-3), {args.reps} alternating "
        f"runs after two warm-ups; gathers of the rows included; SampledSoftmax at m = {M}")
    g = torch.Generator(device=dev).manual_seed(1)
    scale = 3.0 ** 0.5 / D ** 0.25
    users = torch.randn((B, D), generator=g, device=dev) * scale
    items = torch.randn((n_items, D), generator=g, device=dev) * scale
    u_id = torch.randperm(B, generator=g, device=dev)
    ids = (torch.rand(B, generator=g, device=dev) ** 2 * n_items).long().clamp(max=n_items - 1)         # a popular head
    xids = torch.randint(0, n_items, (E,), generator=g, device=dev)
    neg = torch.randint(0, n_items, (B * M,), generator=g, device=dev)
    table = pkg.sampling.item_logq(ids, n_items)
    lq = table[ids]
    xlq = torch.full((E,), -float(np.log(n_items)), device=dev)
    nlq = torch.full((B * M,), -float(np.log(n_items)), device=dev)
    dup = B - int(torch.unique(ids).numel())
    crit = pkg.InBatchSoftmax(WD, B, temperature=TAU)
    sampled = pkg.SampledSoftmax(WD, B, M, temperature=TAU)

    def leaves(*idx):
        return [t.requires_grad_(True) for t in (users[u_id], *(items[i] for i in idx))]

    def fused():
        u, p, x = leaves(ids, xids)
        loss = crit(u, p, item_ids=ids, logq=lq, pos_logq=lq, extra=x, extra_ids=xids, extra_logq=xlq)
        loss.backward()
        return loss.detach()

    def torch_ops():
        u, p, x = leaves(ids, xids)
        loss = torch_ops_loss(u, p, x, ids, xids, lq, xlq, B)
        loss.backward()
        return loss.detach()

    def sampled_m():
        u, p, n = leaves(ids, neg)
        loss = sampled(u, p, n, nlq, lq)
        loss.backward()
        return loss.detach()

    res = compare({"fused in-batch": fused, "torch ops in-batch": torch_ops, f"SampledSoftmax m={M}": sampled_m})
    lf, lt = float(res["fused in-batch"][4]), float(res["torch ops in-batch"][4])
    assert abs(lf - lt) <= 1e-4 * abs(lt), (lf, lt)
    flops = 5 * 2.0 * B * (B + E) * D
    say(f"  {dup} of the {B} rows repeat an earlier row's positive; plan (pieces, column slabs): {pkg.engine.losses.inbatch_softmax_plan(B, E, D)}")
    for k, v in res.items():
        say(f"  {k}: {v[0]:.3f} ms (min {v[1]:.3f}, max {v[2]:.3f}), peak {v[3] / 1e6:.1f} MB on top of the tables"
            + (f", {flops / (v[0] * 1e-3) / 1e12:.1f} TFLOP/s = {100 * flops / (v[0] * 1e-3) / PEAK:.1f} % of the fp32-MFMA peak"
               if k == "fused in-batch" else ""))
    f = res["fused in-batch"][0]
    say(f"  fused / torch ops = {f / res['torch ops in-batch'][0]:.3f}; fused / SampledSoftmax = {f / res[f'SampledSoftmax m={M}'][0]:.3f}")


saved = torch.backends.cuda.matmul.allow_tf32
torch.backends.cuda.matmul.allow_tf32 = False
try:
    lab(512, 0, 260, 100, "the Seoul rows")
    lab(8192, 0, 512, 100000, "C3-sized rows")
    lab(8192, 1024, 512, 100000, "C3-sized rows with extras")
finally:
    torch.backends.cuda.matmul.allow_tf32 = saved
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
