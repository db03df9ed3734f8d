"""BPR against m negatives per positive row (BPRMulti: csrc/bpr_multi.hip) against the two ways round it: the expanded batch through
the existing single-negative kernels (u and p rows repeated m times, BPR(weight_decay, batch_size * m)) and the loss written in
torch ops (abs / logsigmoid / mean and autograd's backward of them).

1. Loss + backward alone on random rows: the Seoul model's D = 260 = 65 x 4 at B = 512, and C3's D = 512 at B = 8 192.
2. The whole training step - forward, loss, backward, optim.Adam - of the Seoul-shaped stand-in (graphs.seoul_standin, 65 -> [65] * 3,
   both dropouts on the device) at B = 512.  The expanded side repeats every id m times.
For m in 1, 4, 8, 24: all sides in one process, alternating, two warm-ups each (the second call of a shape captures the model's
training graphs), device events around each call; medians of --reps runs and the peak device memory on top of what was allocated
before the call.  Writes its lines to --out (default profiles/bpr_multi_lab.txt) as well as to stdout."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

MS = (1, 4, 8, 24)
WD = 0.025

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr_multi_lab.txt"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def torch_ops_loss(u, p, n, m, wd, bs):
    B, D = u.shape
    sp = (u * p).sum(1).abs()
    sn = torch.einsum("bd,bjd->bj", u, n.reshape(B, m, D)).abs()
    rows = -F.logsigmoid(sp[:, None] - sn).mean(1)
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
    f = res["fused"][0]
    say(f"  m = {m:2d}: " + "; ".join(f"{k} {v[0]:.3f} ms (min {v[1]:.3f}, max {v[2]:.3f}, peak {v[3] / 1e6:.1f} MB)" for k, v in res.items())
        + "; " + ", ".join(f"fused / {k} = {f / v[0]:.3f}" for k, v in res.items() if k != "fused"))


def loss_alone(B, D, what):
    say(f"Loss + backward alone, {what}: B = {B}, D = {D}, random rows (scores around +-3), {args.reps} alternating runs after two warm-ups")
    g = torch.Generator(device=dev).manual_seed(1)
    scale = 3.0 ** 0.5 / D ** 0.25
    for m in MS:
        u, p = (torch.randn((B, D), generator=g, device=dev) * scale for _ in range(2))
        n = torch.randn((B * m, D), generator=g, device=dev) * scale
        ue, pe = u.repeat_interleave(m, 0), p.repeat_interleave(m, 0)
        crit_f, crit_e = pkg.BPRMulti(WD, B, m), pkg.BPR(WD, B * m)

        def run(loss_fn, *ops):
            t = [x.detach().requires_grad_(True) for x in ops]
            loss = loss_fn(*t)
            loss.backward()
            return loss.detach()

        res = compare({"fused": lambda: run(crit_f, u, p, n), "expanded": lambda: run(crit_e, ue, pe, n),
                       "torch ops": lambda: run(lambda a, b, c: torch_ops_loss(a, b, c, m, WD, B), u, p, n)})
        lf, le, lt = (float(res[k][4]) for k in ("fused", "expanded", "torch ops"))
        assert abs(lf - le) <= 1e-5 * abs(le) and abs(lf - lt) <= 1e-5 * abs(lt), (lf, le, lt)
        report(m, res)


def training_step(B):
    coo = pkg.graphs.seoul_standin(dev)
    U, I = coo[0]["n_user"], coo[0]["n_item"]
    lap = [pkg.graphs.to_sparse_coo(s) for s in coo]
    num = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    say(f"Whole training step (forward, loss, backward, optim.Adam) on the Seoul-shaped stand-in: {U} users x {I} items, 65 -> [65] * 3, "
        f"B = {B}, node dropout 0.3 and message dropout 0.1 on the device, {args.reps} alternating runs after two warm-ups")
    g = torch.Generator().manual_seed(2)
    r = lambda hi, k: torch.randint(0, hi, (k,), generator=g).to(dev)  # noqa: E731
    for m in MS:
        batch = dict(year=torch.full((B,), 18, device=dev), u_id=r(U, B), age=r(76, B), sex=r(2, B), month=r(13, B), day=r(32, B), dow=r(7, B),
                     pos_item=r(I, B))
        neg = r(I, B * m)
        expanded = {k: v.repeat_interleave(m) for k, v in batch.items()}
        sides = {}
        for name, ids, crit in (("fused", batch, pkg.BPRMulti(WD, B, m)), ("expanded", expanded, pkg.BPR(WD, B * m)),
                                ("torch ops", batch, lambda a, b, c, m=m: torch_ops_loss(a, b, c, m, WD, B))):
            torch.manual_seed(4)
            model = pkg.NGCF(65, [65, 65, 65], 0.3, [0.1, 0.1, 0.1], 1.0, lap, num, B, dev).to(dev)
            model.node_dropout_mode = model.mess_dropout_mode = "device"
            model.train()
            opt = pkg.optim.Adam(model.parameters(), lr=1e-3)

            def step(model=model, opt=opt, ids=ids, crit=crit):
                u, p, n = model(node_flag=True, neg_item=neg, **ids)
                opt.zero_grad()
                loss = crit(u, p, n)
                loss.backward()
                opt.step()
                return loss.detach()

            sides[name] = step
        res = compare(sides)
        assert all(np.isfinite(float(v[4])) for v in res.values())
        report(m, res)


loss_alone(512, 260, "the Seoul model's rows")
loss_alone(8192, 512, "C3's rows")
training_step(512)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
