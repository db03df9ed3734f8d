"""The sampled softmax loss with logQ correction (SampledSoftmax: csrc/sampled_softmax.hip) against its yardstick,
BPRMulti(reduction="softmax") on the same rows (csrc/bpr_multi.hip: the same row machinery, 4 B m bytes of logq fewer to read out of
4 B (m + 2) D), and against the same loss written in torch ops (einsum, subtract, logsumexp and autograd's backward of them).

Loss + backward alone on random rows: the Seoul model's D = 260 = 65 x 4 at B = 512, and C3's D = 512 at B = 8 192, for
m in 1, 8, 24, 64: all sides in one process, alternating, two warm-ups each, device events around each call; medians of --reps runs
and the peak device memory on top of what was allocated before the call (the method of tools/bpr_multi_lab.py).  Writes its lines to
--out (default profiles/sampled_softmax_lab.txt) as well as to stdout."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

MS = (1, 8, 24, 64)
WD, TAU = 0.025, 0.5

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_softmax_lab.txt"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def torch_ops_loss(u, p, n, logq, m, tau, wd, bs):
    B, D = u.shape
    z0 = (u * p).sum(1) / tau
    zj = torch.einsum("bd,bjd->bj", u, n.reshape(B, m, D)) / tau - logq
    rows = torch.logsumexp(torch.cat((z0[:, None], zj), 1), 1) - z0
    return (rows.sum() + wd * (u.pow(2).sum() + p.pow(2).sum() + n.pow(2).sum() / m)) / bs


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


def report(m, res):
    f = res["sampled"][0]
    say(f"  m = {m:2d}: " + "; ".join(f"{k} {v[0]:.3f} ms (min {v[1]:.3f}, max {v[2]:.3f}, peak {v[3] / 1e6:.1f} MB)" for k, v in res.items())
        + "; " + ", ".join(f"sampled / {k} = {f / v[0]:.3f}" for k, v in res.items() if k != "sampled"))


def loss_alone(B, D, what):
    say(f"Loss + backward alone, {what}: B = {B}, D = {D}, random rows (scores around +-3), logq in [-12, 0), temperature {TAU}, "
        f"{args.reps} alternating runs after two warm-ups")
    g = torch.Generator(device=dev).manual_seed(1)
    scale = 3.0 ** 0.5 / D ** 0.25
    for m in MS:
        u, p = (torch.randn((B, D), generator=g, device=dev) * scale for _ in range(2))
        n = torch.randn((B * m, D), generator=g, device=dev) * scale
        logq = -12.0 * torch.rand((B, m), generator=g, device=dev)
        crit_s, crit_m = pkg.SampledSoftmax(WD, B, m, temperature=TAU), pkg.BPRMulti(WD, B, m, "softmax")

        def run(loss_fn):
            t = [x.detach().requires_grad_(True) for x in (u, p, n)]
            loss = loss_fn(*t)
            loss.backward()
            return loss.detach()

        res = compare({"sampled": lambda: run(lambda a, b, c: crit_s(a, b, c, logq)), "multi softmax": lambda: run(crit_m),
                       "torch ops": lambda: run(lambda a, b, c: torch_ops_loss(a, b, c, logq, m, TAU, WD, B))})
        ls, lt = float(res["sampled"][4]), float(res["torch ops"][4])
        assert abs(ls - lt) <= 1e-5 * abs(lt) and np.isfinite(float(res["multi softmax"][4])), (ls, lt)
        report(m, res)


loss_alone(512, 260, "the Seoul model's rows")
loss_alone(8192, 512, "C3's rows")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
