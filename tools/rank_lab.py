"""Full-catalogue ranking lab: ngcf_rank_topk_f32 at the C3, Seoul and demo shapes, against recommend_topk.

    python tools/rank_lab.py [--out profiles/r05_rank_lab.txt] [--skip-c3] [--c3-users N]

C3: synthetic_interactions(1 M, 100 K, 50 M, seed 2603), 20 % of every user's interactions held out, all_E of a 3-layer 128-wide
propagate (D = 512), k = 20, train items excluded; one full ranking of every user timed with device events after a warm-up, then
the metric pass.  The existing path (recommend_topk) is timed on one 8 192-user chunk and extrapolated.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402
from seoul_tourism_recommendation_ngcf_amd import engine as eng  # noqa: E402

PEAK_TF = 157.3          # fp32 matrix peak of the MI355X, TFLOP/s
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=1):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms


def c3(dev, n_users_ranked):
    n_user, n_item, n_inter, seed = 1_000_000, 100_000, 50_000_000, 2603
    t0 = time.time()
    u, i, w = pkg.graphs.synthetic_interactions(n_user, n_item, n_inter, seed=seed, device=dev)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u, i, w, 0.2, seed=seed)
    del u, i, w
    coo = pkg.graphs.bipartite_from_interactions(tu, ti, tw, n_user, n_item)
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(seed)
    model = pkg.NGCF(128, [128, 128, 128], None, None, 1.0, [pkg.graphs.to_sparse_coo(coo)], num_dict, 1024, dev).to(dev).eval()
    del coo
    train = eng.ItemSets.from_pairs(tu, ti, n_user, n_item)
    test = eng.ItemSets.from_pairs(hu, hi, n_user, n_item)
    with torch.no_grad():
        model.propagate(0)
    U, I = model.all_users_emb, model.all_items_emb
    D = int(U.shape[1])
    say(f"C3 set-up {time.time() - t0:.1f} s: {n_user} users x {n_item} items, train {tu.numel()} / held out {hu.numel()} "
        f"interactions, D = {D} (all_E row stride {U.stride(0)}), k = 20, train items excluded")
    ids = torch.arange(n_users_ranked, device=dev)
    out = {}

    def rank():
        out["top"] = eng.rank_topk(U, I, 20, user_ids=ids, exclude=train, status=torch.zeros(1, dtype=torch.int32, device=dev))

    ms = timed(rank)
    flop = 2.0 * n_users_ranked * n_item * D
    tf = flop / (ms * 1e-3) / 1e12
    item_bytes = n_item * D * 4
    tiles = (n_users_ranked + 63) // 64
    say(f"  rank_topk, {n_users_ranked} users: {ms:.1f} ms = {tf:.1f} TFLOP/s = {100 * tf / PEAK_TF:.1f} % of the {PEAK_TF} TFLOP/s "
        f"fp32-matrix peak ({flop:.3e} FLOP)")
    say(f"  item operand bytes per ranking: {tiles} user tiles of 64 x {item_bytes / 1e6:.0f} MB = {tiles * item_bytes / 1e12:.2f} TB "
        f"= {tiles * item_bytes / (ms * 1e-3) / 1e12:.2f} TB/s over the run (L2 / MALL, the table is read once per tile)")
    sums = torch.zeros(5, dtype=torch.float64, device=dev)

    def metrics():
        sums.zero_()
        eng.ranking_metrics(out["top"][1], test, [20], user_ids=ids, sums=sums)

    mm = timed(metrics)
    say(f"  ranking_metrics over {n_users_ranked} users: {mm:.2f} ms; {eng.metrics_from_sums(sums, [20])}")
    # the existing path on one 8 192-user chunk (score matrix in HBM + radix select), extrapolated
    chunk = U[:8192]
    mr = timed(lambda: eng.recommend_topk(chunk, I, 20))
    say(f"  recommend_topk, one 8192-user chunk (no exclusion): {mr:.1f} ms -> EXTRAPOLATED to {n_user} users: "
        f"{mr * n_user / 8192 / 1e3:.1f} s (plus a {8192 * n_item * 4 / 1e9:.1f} GB score scratch per chunk)")
    if n_users_ranked >= 8192:
        mc = timed(lambda: eng.rank_topk(chunk, I, 20))
        say(f"  rank_topk on the same chunk (no exclusion): {mc:.2f} ms")


def small(dev, name, B, n_items, D, k, reps):
    g = torch.Generator(device=dev).manual_seed(B + n_items)
    u = torch.randn((B, D), generator=g, device=dev)
    items = torch.randn((n_items, D), generator=g, device=dev)
    tn = timed(lambda: eng.rank_topk(u, items, k), reps) * 1e3
    to = timed(lambda: eng.recommend_topk(u, items, k), reps) * 1e3
    ws = int(pkg._lib.load().ngcf_rank_workspace_bytes(B, n_items, D, k))
    say(f"{name}: B = {B}, {n_items} items, D = {D}, k = {k}: rank_topk {tn:.1f} us/call, recommend_topk {to:.1f} us/call "
        f"(rank workspace {ws} B: {'item-split path' if ws else 'one launch'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--c3-users", type=int, default=1_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say(f"rank_lab on {torch.cuda.get_device_name(0)}")
    small(dev, "Seoul shape", 5840, 100, 193, 20, 20)
    small(dev, "Demo shape", 4, 100_000, 193, 100, 20)
    small(dev, "Demo shape, D = 512", 4, 100_000, 512, 100, 20)
    if not args.skip_c3:
        c3(dev, args.c3_users)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
