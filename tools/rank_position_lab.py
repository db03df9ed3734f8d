"""Exact held-out positions lab: evaluate.full_ranks against evaluate.full_ranking and against torch.

    python tools/rank_position_lab.py [--out profiles/rank_position_lab.txt] [--skip-c3] [--c3-users N]

C3: synthetic_interactions(1 M, 100 K, 50 M, seed 2603), 20 % of every user's interactions held out (graphs.holdout_split), all_E of
a 3-layer 128-wide propagate (D = 512), train items excluded.  Each path is run once to warm up and then timed with device events;
the reference point, full_ranking(ks=(20,)), runs on the same tables in the same process.  The torch formulation (a chunk of the
score matrix, compare with the held-out scores, sum) is timed on one chunk of users and extrapolated.
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


def torch_positions(U, I, ids, truth, excl):
    """The torch formulation for the users `ids`: their rows of the score matrix, the excluded entries at -inf, and per held-out
    item the number of scores above it (ties by item id).  Memory: len(ids) x n_items floats, and as much again per compare."""
    s = U[ids] @ I.T
    rp, ci = excl.rowptr, excl.colidx.long() - excl.col_offset
    rows = torch.repeat_interleave(torch.arange(ids.numel(), device=U.device), rp[ids + 1] - rp[ids])
    s[rows, torch.cat([ci[rp[r]:rp[r + 1]] for r in ids.tolist()])] = float("-inf")
    out = []
    trp, tci = truth.rowptr, truth.colidx.long() - truth.col_offset
    item = torch.arange(I.shape[0], device=U.device)
    for b, r in enumerate(ids.tolist()):
        t = tci[trp[r]:trp[r + 1]]
        st = s[b, t]
        above = (s[b][None, :] > st[:, None]) | ((s[b][None, :] == st[:, None]) & (item[None, :] < t[:, None]))
        out.append(above.sum(1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64, device=U.device)


def compare(dev, name, model, train, test, n_users_ranked, torch_chunk):
    with torch.no_grad():
        model.propagate(0)
    U, I = model.all_users_emb, model.all_items_emb
    n_user, n_item, D = int(U.shape[0]), int(I.shape[0]), int(U.shape[1])
    ids = torch.arange(n_users_ranked, device=dev)
    rp = test.rowptr
    n_held = int(rp[n_users_ranked] - rp[0])
    with_rows = int((rp[1:n_users_ranked + 1] > rp[:n_users_ranked]).sum())
    longest = int(rp.diff()[:n_users_ranked].max())
    say(f"{name}: {n_users_ranked} of {n_user} users x {n_item} items, D = {D}; {n_held} held-out entries on {with_rows} users, "
        f"longest row {longest} (rows are ranked {eng.ranks.POSITION_CAP} entries at a time)")
    res = {}
    t_ref = timed(lambda: res.__setitem__("ref", pkg.evaluate.full_ranking(model, train, test, ks=(20,), users=ids)))
    t_new = timed(lambda: res.__setitem__("new", pkg.evaluate.full_ranks(model, train, test, ks=(20,), users=ids)))
    flop = 2.0 * with_rows * n_item * D
    say(f"  full_ranking(ks=(20,)): {t_ref:.1f} ms (propagate included)   {res['ref']}")
    say(f"  full_ranks(ks=(20,)):   {t_new:.1f} ms (propagate included)   {res['new']}")
    say(f"  ratio full_ranks / full_ranking = {t_new / t_ref:.2f}; {flop / (t_new * 1e-3) / 1e12:.1f} TFLOP/s over the users with held-out "
        f"items = {100 * flop / (t_new * 1e-3) / 1e12 / PEAK_TF:.1f} % of the fp32-matrix peak")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    buf = torch.full((int(test.colidx.numel()),), -2, dtype=torch.int32, device=dev)
    chunk = ids[:65536]
    t_pos = timed(lambda: eng.ranks.rank_positions(U, I, test, user_ids=chunk, exclude=train, out=buf, status=status))
    t_top = timed(lambda: eng.rank_topk(U, I, 20, user_ids=chunk, exclude=train, status=status))
    sums = torch.zeros(10, dtype=torch.float64, device=dev)
    t_met = timed(lambda: eng.ranks.position_metrics(buf, test, (20,), n_item, exclude=train, user_ids=chunk, sums=sums, status=status))
    say(f"  one chunk of {chunk.numel()} users: rank_positions {t_pos:.2f} ms, rank_topk(k=20) {t_top:.2f} ms, position_metrics {t_met:.3f} ms")
    few = ids[:torch_chunk]
    want = {}
    t_torch = timed(lambda: want.__setitem__("p", torch_positions(U, I, few, test, train)))
    got = eng.ranks.rank_positions(U, I, test, user_ids=few, exclude=train, status=status)[int(rp[0]):int(rp[torch_chunk])]
    agree = float((got.long() == want["p"]).double().mean()) if got.numel() else 1.0
    say(f"  torch (score rows, compare, sum), {torch_chunk} users: {t_torch:.1f} ms -> EXTRAPOLATED to {n_users_ranked} users: "
        f"{t_torch * n_users_ranked / torch_chunk / 1e3:.2f} s; positions equal on {100 * agree:.2f} % of the entries (torch.mm sums in "
        f"another order, so near-ties may differ)")


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
    say(f"C3 set-up {time.time() - t0:.1f} s")
    compare(dev, "C3", model, train, test, n_users_ranked, 256)


def seoul(dev):
    n_user, n_item = 5840, 100
    u, i, w = pkg.graphs.synthetic_interactions(n_user, n_item, 438_000, seed=7, device=dev)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u, i, w, 0.2, seed=7)
    coo = pkg.graphs.bipartite_from_interactions(tu, ti, tw, n_user, n_item)
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(7)
    model = pkg.NGCF(65, [64, 64], None, None, 1.0, [pkg.graphs.to_sparse_coo(coo)], num_dict, 256, dev).to(dev).eval()
    train = eng.ItemSets.from_pairs(tu, ti, n_user, n_item)
    test = eng.ItemSets.from_pairs(hu, hi, n_user, n_item)
    compare(dev, "Seoul shape", model, train, test, n_user, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rank_position_lab.txt")
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--c3-users", type=int, default=1_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say(f"rank_position_lab on {torch.cuda.get_device_name(0)}")
    seoul(dev)
    if not args.skip_c3:
        c3(dev, args.c3_users)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
