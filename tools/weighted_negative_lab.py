"""Popularity-weighted negatives (engine.negatives.weighted_unseen: one launch over prepared integer arrays) beside the uniform
sampler it sits next to and against the torch formulation it replaces.

1. C3's catalogue (bench.py's 1 M users x 100 K items with the popular head, ~50 M positives), weights popularity^0.75.
2. The Seoul-shaped stand-in (graphs.seoul_standin: 5 840 users x 100 items, every positive row).  Its seen rows are about 75 of 100
   items long, so at m = 32 most users have too few unseen items: only the rows that can draw are drawn, by every side, and their
   share is reported.
For m in 1, 8, 32, in one process per shape, alternating, medians of --reps runs after one warm-up each, device events around each
call:
  weighted   engine.negatives.weighted_unseen over all rows, and once more over the rows the torch side gets
  uniform    engine.sample_unseen over all rows at the same m
  torch      for chunks of rows: a [chunk, n_items] fp32 matrix of the weights, the users' seen items set to 0, torch.multinomial
             without replacement - over the first --torch-rows rows only (the whole of C3 would take hours); its time is also
             given per million rows next to the weighted draw's over the same rows
with the peak device memory each side takes on top of the inputs, and the time of WeightedSets (cumsum, ngcf_weighted_prepare, the
read-back).  Each shape runs in a child process of its own under a time limit; the first one that fails or runs out of time ends
the tool.  Writes its lines to --out (default profiles/weighted_negative_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 8, 32)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_negative_lab.txt"))
ap.add_argument("--interactions", type=int, default=50_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-rows", type=int, default=32768, help="rows the torch formulation draws for")
ap.add_argument("--torch-chunk", type=int, default=4096, help="rows of one [chunk, n_items] probability matrix")
ap.add_argument("--step-timeout", type=int, default=400, help="seconds for one shape")
ap.add_argument("--step", default=None, help="internal: the one shape this process measures")
args = ap.parse_args()


def driver():
    lines = []
    for shape in ("c3", "seoul"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", shape, "--interactions", str(args.interactions), "--reps", str(args.reps),
               "--torch-rows", str(args.torch_rows), "--torch-chunk", str(args.torch_chunk)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"weighted_negative_lab: {shape} ran out of its {args.step_timeout} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            sys.stderr.write(res.stderr)
            sys.exit(f"weighted_negative_lab: {shape} ended with status {res.returncode}; nothing more is started")
        lines += [ln for ln in res.stdout.splitlines() if ln.startswith(("C3", "Seoul", "  "))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def step(shape):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng, sampling = pkg.engine, pkg.sampling
    dev = torch.device("cuda:0")
    if shape == "c3":
        NU, NI = 1_000_000, 100_000
        users, items, _ = pkg.graphs.synthetic_interactions(NU, NI, args.interactions, seed=2603, device=dev)
        name = "C3's catalogue"
    else:
        coo = pkg.graphs.seoul_standin(dev)[0]
        NU, NI = coo["n_user"], coo["n_item"]
        sel = coo["rows"] < NU
        users, items = coo["rows"][sel].to(torch.int64).contiguous(), (coo["cols"][sel] - NU).to(torch.int64).contiguous()
        name = "Seoul-shaped stand-in"
    seen = eng.ItemSets.from_pairs(users, items, NU, NI)
    weights = sampling.popularity_weights(items, NI, alpha=0.75)
    w32 = weights.to(torch.float32)
    positive = int((weights > 0).sum())
    row_len = seen.rowptr.diff()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    key = torch.unique(users * NI + items)                                    # the (user, item) pairs that count as seen

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

    def median_of(fns):
        """Medians, extremes and peaks of several callables, run alternately after one warm-up each."""
        for fn in fns:
            measure(fn)
        times, peaks = [[] for _ in fns], [0 for _ in fns]
        for _ in range(args.reps):
            for k, fn in enumerate(fns):
                ms, pk, _ = measure(fn)
                times[k].append(ms)
                peaks[k] = max(peaks[k], pk)
        return [(float(np.median(t)), min(t), max(t), pk) for t, pk in zip(times, peaks)]

    (prep, prep_lo, prep_hi, prep_peak), = median_of([lambda: eng.negatives.WeightedSets(seen, weights)])
    wsets = eng.negatives.WeightedSets(seen, weights)
    print(f"{name}: {NU} users x {NI} items ({positive} of positive weight, weights popularity^0.75 at resolution 1024, W = {wsets.total}), "
          f"T = {int(users.numel())} positive rows; WeightedSets (cumsum, prepare, read-back) {prep:.3f} ms (min {prep_lo:.3f}, max {prep_hi:.3f}), "
          f"its arrays {(wsets.cdf.numel() + wsets.gap.numel() + wsets.mass.numel()) * 8 / 1e6:.1f} MB; {args.reps} alternating runs after one warm-up each")

    for m in MS:
        can = row_len[users] <= positive - m                                  # the seen items all have positive weight: they are counts
        share = float(can.double().mean())
        rows = users[can].contiguous()
        T = int(rows.numel())
        if T == 0:
            print(f"  m = {m:2d}: no row has {m} unseen items of positive weight")
            continue
        sub = rows[:args.torch_rows].contiguous()
        Ts = int(sub.numel())

        def weighted():
            return eng.negatives.weighted_unseen(wsets, rows, m, 2024, status=status)

        def weighted_sub():
            return eng.negatives.weighted_unseen(wsets, sub, m, 2024, status=status)

        def uniform():
            return eng.sample_unseen(seen, rows, m, 2024, status=status)

        def torch_side():
            out = torch.empty((Ts, m), dtype=torch.int64, device=dev)
            for r0 in range(0, Ts, args.torch_chunk):
                u = sub[r0:r0 + args.torch_chunk]
                p = w32.expand(int(u.numel()), NI).contiguous()
                lens = row_len[u]
                row_of = torch.repeat_interleave(torch.arange(int(u.numel()), device=dev), lens)
                first = seen.rowptr[u]
                pos = torch.arange(int(row_of.numel()), device=dev) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
                p[row_of, seen.colidx[first[row_of] + pos].long()] = 0
                out[r0:r0 + args.torch_chunk] = torch.multinomial(p, m, replacement=False)
            return out

        (w_ms, w_lo, w_hi, w_pk), (s_ms, s_lo, s_hi, s_pk), (u_ms, u_lo, u_hi, u_pk), (t_ms, t_lo, t_hi, t_pk) = median_of(
            [weighted, weighted_sub, uniform, torch_side])
        neg = weighted_sub()
        clean =not bool(torch.isin(sub[:, None] * NI + neg, key).any()) and not bool(torch.isin(sub[:, None] * NI + torch_side(), key).any())
        print(f"  m = {m:2d}: {T} rows draw ({100 * share:.1f} %): weighted {w_ms:.3f} ms (min {w_lo:.3f}, max {w_hi:.3f}, peak {w_pk / 1e6:.1f} MB), "
              f"uniform sample_unseen {u_ms:.3f} ms (min {u_lo:.3f}, max {u_hi:.3f}, peak {u_pk / 1e6:.1f} MB), weighted / uniform = {w_ms / u_ms:.3f}; "
              f"over the first {Ts} rows: weighted {s_ms:.3f} ms (min {s_lo:.3f}, max {s_hi:.3f}, peak {s_pk / 1e6:.1f} MB), torch.multinomial in chunks of "
              f"{args.torch_chunk} {t_ms:.3f} ms (min {t_lo:.3f}, max {t_hi:.3f}, peak {t_pk / 1e6:.1f} MB), weighted / torch = {s_ms / t_ms:.5f}; per million "
              f"rows: weighted {w_ms / T * 1e6:.3f} ms over all rows, torch {t_ms / Ts * 1e6:.1f} ms; no side drew a seen item: {clean}")
        assert clean, "a drawn item is in its user's seen row"
    assert int(status.item()) == 0, "a row that should draw did not"


if args.step is None:
    driver()
else:
    step(args.step)
