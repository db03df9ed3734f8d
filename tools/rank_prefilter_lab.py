"""Lab of the certified two-stage ranking (engine.shortlist, csrc/rank_prefilter.hip) against engine.rank_topk on the same tables, both
sides in one process, alternating, medians of 5 after two warm-ups -> profiles/rank_prefilter_lab.txt.

  python tools/rank_prefilter_lab.py                       # the Seoul shape and a C3-sized table cut to --users rows
  python tools/rank_prefilter_lab.py --users 1000000       # all of C3's users (minutes)

Per shape and pool: rank_topk ms, rank_topk_certified ms (pack, shortlist, re-score and fallback) and their ratio, the certified
share, the bytes the re-score gathers, and on a small cut the measured error of the bf16 scores over beta."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seoul_tourism_recommendation_ngcf_amd import engine, graphs  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def shape(name, n_user, n_item, D, k, nnz, pools, lines):
    g = torch.Generator(device=DEV).manual_seed(1)
    U = torch.randn((n_user, D), generator=g, device=DEV) * 0.1
    I = torch.randn((n_item, D), generator=g, device=DEV) * 0.1  # noqa: E741
    u_, i_, _ = graphs.synthetic_interactions(n_user, n_item, nnz, seed=2, device=DEV)
    excl = engine.ItemSets.from_pairs(u_, i_, n_user, n_item)
    sides = {"rank_topk": lambda: engine.rank_topk(U, I, k, exclude=excl)}
    for pool in pools:
        sides[f"certified pool={pool}"] = (lambda pool=pool: engine.shortlist.rank_topk_certified(U, I, k, exclude=excl, pool=pool,
                                                                                                  return_certified=True))
    times = {s: [] for s in sides}
    last = {}
    for rep in range(7):
        for s, fn in sides.items():
            ms, last[s] = timed(fn)
            if rep >= 2:
                times[s].append(ms)
    base = statistics.median(times["rank_topk"])
    lines.append(f"{name}: {n_user} users x {n_item} items, D = {D}, k = {k}, {int(excl.colidx.numel())} exclusions")
    lines.append(f"  rank_topk                 {base:10.3f} ms")
    for pool in pools:
        s = f"certified pool={pool}"
        v, i, cert = last[s]
        same = torch.equal(v.view(torch.int32), last["rank_topk"][0].view(torch.int32)) and torch.equal(i, last["rank_topk"][1])
        med = statistics.median(times[s])
        lines.append(f"  {s:<25s} {med:10.3f} ms   ratio {med / base:6.3f}   certified {float(cert.float().mean()):.4f}   "
                     f"re-score gathers {n_user * pool * D * 4 / 1e9:.2f} GB   equal to rank_topk: {same}")
    cut_u, cut_i = U[:64], I[:4096]
    approx, _ = engine.shortlist.shortlist_scores(cut_u, cut_i)
    s64 = cut_u.double().cpu() @ cut_i.double().cpu().T
    norms = cut_u.double().norm(dim=1).cpu()[:, None] * cut_i.double().norm(dim=1).cpu()[None, :]
    err = float(((approx.double().cpu() - s64).abs() / norms).max())
    lines.append(f"  measured |s~ - s_fp64| / (|u||i|), 64 users x {cut_i.shape[0]} items: {err:.3e} = {err / engine.shortlist.beta(D):.4f} beta")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=131072, help="rows of the C3-sized user table (C3: 1 000 000)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rank_prefilter_lab.txt"))
    a = ap.parse_args()
    lines = ["rank_prefilter_lab: engine.shortlist.rank_topk_certified against engine.rank_topk, one process, alternating, median of 5 "
             "after 2 warm-ups", f"device: {torch.cuda.get_device_name(0)}", ""]
    shape("Seoul shape", 5840, 100, 260, 20, 876000 // 2, (64, 128, 256), lines)
    lines.append("")
    shape("C3-sized", a.users, 100000, 512, 20, a.users * 50, (64, 128, 256), lines)
    lines += ["", "open: the certified share on a trained model's embeddings (norms and score gaps differ from these Gaussian tables);",
              "      the per-stage split (run this tool under a kernel trace of its own)."]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    np.random.seed(0)
    main()
