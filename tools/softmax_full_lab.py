"""The softmax loss over the whole catalogue (SoftmaxFull: csrc/softmax_full.hip) against the same loss written in torch ops (`mm`,
`logsumexp`, autograd; chunked over B so that its [chunk, n_items] score matrix and the gradient of the same size fit).

1. Loss + backward alone on random rows: C3-sized rows (B = 8 192, 100 000 items, D = 512) and the Seoul shape (B = 512, 100 items,
   D = 260).  Time, peak device memory on top of the inputs, and the achieved share of the fp32-MFMA peak (157.3 TFLOP/s), taking
   5 x 2 B n_items D flops for forward plus backward (one score pass forward, score pass + accumulation for each gradient).
2. The whole eager training step - forward, loss, backward, optim.Adam - of the Seoul-shaped stand-in (graphs.seoul_standin,
   65 -> [65] * 3, both dropouts on the device, auto_train_graph off on both sides) at B = 512 with `BPR` against `SoftmaxFull`.
Both sides in one process, alternating, two warm-ups each, device events around each call; medians of --reps runs.  Writes its lines
to --out (default profiles/softmax_full_lab.txt) as well as to stdout."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

WD, TAU, PEAK = 0.025, 1.0, 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_full_lab.txt"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--chunk", type=int, default=1024, help="rows of B per chunk of the torch-op side")
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def torch_ops_step(u, items, pos, wd, bs, chunk):
    """Loss and both gradients in torch ops, chunk rows of B at a time (the chunks' item gradients accumulate in `.grad`)."""
    tu, ti = u.detach().requires_grad_(True), items.detach().requires_grad_(True)
    total = torch.zeros((), device=u.device)
    for b0 in range(0, u.shape[0], chunk):
        uc, pc = tu[b0:b0 + chunk], pos[b0:b0 + chunk]
        s = torch.mm(uc, ti.t()) * (1.0 / TAU)
        loss = ((torch.logsumexp(s, 1) - s.gather(1, pc[:, None])[:, 0]).sum() + wd * (uc.pow(2).sum() + ti[pc].pow(2).sum())) / bs
        loss.backward()
        total += loss.detach()
    return total


def fused_step(crit, u, items, pos):
    tu, ti = u.detach().requires_grad_(True), items.detach().requires_grad_(True)
    loss = crit(tu, pos, ti)
    loss.backward()
    return loss.detach()


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


def loss_alone(B, n_items, D, what):
    say(f"Loss + backward alone, {what}: B = {B}, {n_items} items, D = {D}, random rows (scores around +-3), {args.reps} alternating runs "
        f"after two warm-ups; torch ops in chunks of {min(args.chunk, B)} rows, TF32 off")
    g = torch.Generator(device=dev).manual_seed(1)
    scale = 3.0 ** 0.5 / D ** 0.25
    u = torch.randn((B, D), generator=g, device=dev) * scale
    items = torch.randn((n_items, D), generator=g, device=dev) * scale
    pos = torch.randint(0, n_items, (B,), generator=g, device=dev)
    crit = pkg.SoftmaxFull(WD, B, temperature=TAU, check_indices=False)
    res = compare({"fused": lambda: fused_step(crit, u, items, pos),
                   "torch ops": lambda: torch_ops_step(u, items, pos, WD, B, args.chunk)})
    lf, lt = float(res["fused"][4]), float(res["torch ops"][4])
    assert abs(lf - lt) <= 1e-4 * abs(lt), (lf, lt)
    flops = 5 * 2.0 * B * n_items * D
    plan = pkg.engine.losses.softmax_full_plan(B, n_items, D)
    say(f"  plan (pieces, column slabs): {plan}")
    for k, v in res.items():
        say(f"  {k}: {v[0]:.3f} ms (min {v[1]:.3f}, max {v[2]:.3f}), peak {v[3] / 1e6:.1f} MB on top of the inputs"
            + (f", {flops / (v[0] * 1e-3) / 1e12:.1f} TFLOP/s = {100 * flops / (v[0] * 1e-3) / PEAK:.1f} % of the fp32-MFMA peak" if k == "fused" else ""))
    say(f"  fused / torch ops = {res['fused'][0] / res['torch ops'][0]:.3f}")


def training_step(B):
    coo = pkg.graphs.seoul_standin(dev)
    U, I = coo[0]["n_user"], coo[0]["n_item"]
    lap = [pkg.graphs.to_sparse_coo(s) for s in coo]
    num = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    say(f"Whole eager training step (forward, loss, backward, optim.Adam) on the Seoul-shaped stand-in: {U} users x {I} items, "
        f"65 -> [65] * 3, B = {B}, node dropout 0.3 and message dropout 0.1 on the device, auto_train_graph off, {args.reps} alternating "
        "runs after two warm-ups")
    g = torch.Generator().manual_seed(2)
    r = lambda hi, k: torch.randint(0, hi, (k,), generator=g).to(dev)  # noqa: E731
    batch = dict(year=torch.full((B,), 18, device=dev), u_id=r(U, B), age=r(76, B), sex=r(2, B), month=r(13, B), day=r(32, B), dow=r(7, B),
                 pos_item=r(I, B))
    neg = r(I, B)
    none = torch.empty(0, dtype=torch.int64, device=dev)
    sides = {}
    for name in ("BPR", "SoftmaxFull"):
        torch.manual_seed(4)
        model = pkg.NGCF(65, [65, 65, 65], 0.3, [0.1, 0.1, 0.1], 1.0, lap, num, B, dev).to(dev)
        model.node_dropout_mode = model.mess_dropout_mode = "device"
        model.auto_train_graph = False
        model.train()
        opt = pkg.optim.Adam(model.parameters(), lr=1e-3)
        crit = pkg.BPR(WD, B) if name == "BPR" else pkg.SoftmaxFull(WD, B, check_indices=False)

        def step(model=model, opt=opt, crit=crit, name=name):
            u, p, n = model(node_flag=True, neg_item=neg if name == "BPR" else none, **batch)
            opt.zero_grad()
            loss = crit(u, p, n) if name == "BPR" else crit(u, batch["pos_item"], model.all_items_emb)
            loss.backward()
            opt.step()
            return loss.detach()

        sides[name] = step
    res = compare(sides)
    assert all(np.isfinite(float(v[4])) for v in res.values())
    say("  " + "; ".join(f"{k} {v[0]:.3f} ms (min {v[1]:.3f}, max {v[2]:.3f}, peak {v[3] / 1e6:.1f} MB)" for k, v in res.items())
        + f"; SoftmaxFull / BPR = {res['SoftmaxFull'][0] / res['BPR'][0]:.3f}")


saved = torch.backends.cuda.matmul.allow_tf32
torch.backends.cuda.matmul.allow_tf32 = False
try:
    loss_alone(512, 100, 260, "the Seoul shape")
    loss_alone(8192, 100000, 512, "C3-sized rows")
    training_step(512)
finally:
    torch.backends.cuda.matmul.allow_tf32 = saved
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
