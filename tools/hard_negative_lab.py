"""Hard negatives (engine.negatives.hard_unseen: draw, score and select in one launch) against the composition of the kernels it
fuses: engine.sample_unseen, engine.eval_candidates(return_scores=True), an argmax and a gather - which writes the [T, m] int64
candidates and the [T, m] fp32 scores to memory.

1. C3's tables (bench.py's 1 M users x 100 K items, D = 512 = 128 + 3 x 128, ~50 M positives).
2. The Seoul-shaped stand-in (graphs.seoul_standin: 5 840 users x 100 items, D = 193 = 65 + 64 + 64, every positive row).  Its seen
   rows are about 75 of 100 items long, so at m = 32 most users have too few unseen items and draw nothing: the share of rows that
   draw is reported, and both sides skip the same rows.
For m in 2, 8, 32: both sides on the same tables, seen sets and rows in one process, alternating, one warm-up each, device events
around each call; the items of both sides are compared.  Reported per configuration: the median ms of both and their ratio,
T * m * D * 4 bytes of gathered item rows per second, and the peak device memory each side takes on top of the inputs.

Every (shape, m) runs in a child process of its own under a time limit, one after the other; the first one that fails or runs out
of time ends the tool.  Writes its lines to --out (default profiles/hard_negative_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (2, 8, 32)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_negative_lab.txt"))
ap.add_argument("--interactions", type=int, default=50_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=240, help="seconds for one (shape, m)")
ap.add_argument("--step", default=None, help="internal: <shape>:<m>, the one configuration this process measures")
args = ap.parse_args()


def driver():
    lines = []
    for shape in ("c3", "seoul"):
        for m in MS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{shape}:{m}", "--interactions", str(args.interactions),
                   "--reps", str(args.reps)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                sys.exit(f"hard_negative_lab: {shape} m={m} ran out of its {args.step_timeout} s; nothing more is started")
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            if res.returncode != 0:
                sys.stderr.write(res.stderr)
                sys.exit(f"hard_negative_lab: {shape} m={m} ended with status {res.returncode}; nothing more is started")
            lines += [ln for ln in res.stdout.splitlines() if ln.startswith(("C3", "Seoul", "  "))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def step(shape, m):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = pkg.engine
    dev = torch.device("cuda:0")
    gd = torch.Generator(device=dev).manual_seed(3)
    if shape == "c3":
        NU, NI, D = 1_000_000, 100_000, 512
        users, items, _ = pkg.graphs.synthetic_interactions(NU, NI, args.interactions, seed=2603, device=dev)
        name = "C3's tables"
    else:
        coo = pkg.graphs.seoul_standin(dev)[0]
        NU, NI, D = coo["n_user"], coo["n_item"], 193
        sel = coo["rows"] < NU
        users, items = coo["rows"][sel].to(torch.int64).contiguous(), (coo["cols"][sel] - NU).to(torch.int64).contiguous()
        name = "Seoul-shaped stand-in"
    all_E = torch.randn((NU + NI, D), generator=gd, device=dev) * 0.1
    U, I = all_E[:NU], all_E[NU:]
    seen = eng.ItemSets.from_pairs(users, items, NU, NI)
    T = int(users.numel())
    draws = float((seen.rowptr.diff()[users] <= NI - m).double().mean())
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)

    def fused():
        return eng.negatives.hard_unseen(seen, U, I, users, m, 2024, status=status)

    def composed():
        cand = eng.sample_unseen(seen, users, m, 2024, status=status)   # a row that draws nothing holds -1: eval_candidates skips it too
        scores = eng.eval_candidates(U, I, users, cand, ks=(), hit_k=1, sums=sums, status=status, return_scores=True, return_position=False)[2]
        return cand.gather(1, scores.argmax(1, keepdim=True))[:, 0]

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

    measure(fused), measure(composed)                          # warm-up: code objects, the allocator's blocks
    t_f, t_c, peak_f, peak_c = [], [], 0, 0
    for _ in range(args.reps):                                 # alternating: both sides see the same machine
        ms, pk, neg_f = measure(fused)
        t_f.append(ms)
        peak_f = max(peak_f, pk)
        ms, pk, neg_c = measure(composed)
        t_c.append(ms)
        peak_c = max(peak_c, pk)
    drew = neg_f >= 0
    same = bool((neg_f[drew] == neg_c[drew]).all())
    del neg_c
    med_f, med_c = float(np.median(t_f)), float(np.median(t_c))
    gb = T * draws * m * D * 4 / 1e9
    if m == MS[0]:
        print(f"{name}: {NU} users x {NI} items ({NI * D * 4 / 1e6:.1f} MB of item rows), D = {D}, T = {T} positive rows, "
              f"uniformly random tables, {args.reps} alternating runs after one warm-up each")
    print(f"  m = {m:2d}: fused {med_f:.3f} ms (min {min(t_f):.3f}, max {max(t_f):.3f}), composition {med_c:.3f} ms (min {min(t_c):.3f}, "
          f"max {max(t_c):.3f}), fused / composition = {med_f / med_c:.3f}; {gb:.2f} GB of gathered item rows -> fused {gb / med_f:.2f} TB/s, "
          f"composition {gb / med_c:.2f} TB/s; peak memory on top of the inputs: fused {peak_f / 1e6:.1f} MB, composition {peak_c / 1e6:.1f} MB; "
          f"rows that draw: {100 * draws:.1f} %; items equal: {same}")
    assert same, "the fused call and the composition chose different items"


if args.step is None:
    driver()
else:
    step(args.step.split(":")[0], int(args.step.split(":")[1]))
