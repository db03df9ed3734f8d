"""Trip recommendation (recommend.blended_ranking / engine.blend_points) against the routes it replaces, for R = 65 536 request rows
in G = 16 384 columns (4 rows each), P = 100 point ranks, three kinds of points, half the items masked, top 10.

1. Seoul-shaped graph (graphs.seoul_standin: 5 840 users x 100 items, embed 65 -> [64, 64]): one blended_ranking call; the same
   result with torch ops on the same device (mm, topk, scatter_add_ into dense [G, n_item] tables, topk); and the per-row loop of
   the reference's shape (demo.py:260-313: per request row three indexed `rating += rank2rate * weight`, here on device tensors
   in place of data frames), timed on --loop-rows rows and scaled.
2. C3-sized tables (1 M users, 100 K items, D = 512): rank_topk + 2 topk_rows + blend_points as blended_ranking runs them, against
   the dense torch route.

Timed with device events around work that ends in a synchronise, one warm-up run, --reps runs, median (min, max).
Writes its lines to --out (default profiles/blend_lab.txt) as well as to stdout."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_lab.txt"))
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--loop-rows", type=int, default=2048)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-big", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
eng = pkg.engine
R, P, TOP, W = args.rows, 100, 10, (0.5, 0.3, 0.2)
G = R // 4
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def fmt(ms):
    return f"median {np.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)"


def inputs(n_user, n_item, gen):
    uid = torch.randint(0, n_user, (R,), generator=gen, device=dev)
    number = torch.arange(R, device=dev) // 4                         # 4 request rows per column
    con = torch.rand((31, n_item), generator=gen, device=dev)
    dist = torch.rand((8, n_item), generator=gen, device=dev) * 2e4
    con_slot = torch.randint(0, 31, (R,), generator=gen, device=dev)
    dis_slot = torch.randint(0, 8, (R,), generator=gen, device=dev)
    mask = torch.rand((n_item,), generator=gen, device=dev) < 0.5
    return uid, number, con, dist, con_slot, dis_slot, mask


def torch_route(users, items, uid, number, con, dist, con_slot, dis_slot, mask, row_chunk=R):
    """The same ratings with torch ops: topk lists, scatter_add_ of the points into dense [G, n_item] int64 tables, the fp64
    formula, the mask, topk (whose order among equal ratings is not specified: ratings are compared, not items)."""
    n_item = int(items.shape[0])
    Pl = min(P, n_item)
    pts = torch.arange(P, P - Pl, -1, device=dev, dtype=torch.int64)
    tabs = [torch.zeros((G, n_item), dtype=torch.int64, device=dev) for _ in range(3)]
    con_l = torch.topk(-con, Pl, dim=1).indices
    dis_l = torch.topk(-dist, Pl, dim=1).indices
    for c0 in range(0, R, row_chunk):
        sl = slice(c0, c0 + row_chunk)
        pref = torch.topk(users[uid[sl]] @ items.T, Pl, dim=1).indices
        col = number[sl, None].expand(-1, Pl)
        for tab, lists in zip(tabs, (pref, con_l[con_slot[sl]], dis_l[dis_slot[sl]])):
            tab.view(-1).scatter_add_(0, (col * n_item + lists).reshape(-1), pts.expand(lists.shape[0], -1).reshape(-1))
    rating = (tabs[0].double() * W[0] + tabs[1].double() * W[1]) + tabs[2].double() * W[2]
    rating.masked_fill_(~mask[None, :], float("-inf"))
    return torch.topk(rating, TOP, dim=1)


# ---- 1. Seoul-shaped graph ---------------------------------------------------------------------------------------------------
slices = pkg.graphs.seoul_standin(dev)
U, I = slices[0]["n_user"], slices[0]["n_item"]
num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
torch.manual_seed(1801)
model = pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, [pkg.graphs.to_sparse_coo(s) for s in slices], num_dict, 25, dev).to(dev).eval()
gd = torch.Generator(device=dev).manual_seed(3)
uid, number, con, dist, con_slot, dis_slot, mask = inputs(U, I, gd)
call = lambda: pkg.recommend.blended_ranking(model, uid, columns=number, weights=W, congestion=con, congestion_slot=con_slot,  # noqa: E731
                                             distance=dist, distance_slot=dis_slot, item_mask=mask, top=TOP, points=P)
t_call = timed(call, args.reps)
items_k, rating_k = call()
with torch.no_grad():
    model.propagate(0)
    users_t, items_t = model.all_users_emb, model.all_items_emb
    _, pref = eng.rank_topk(users_t, items_t, P, user_ids=uid)
    _, con_l = eng.topk_rows(-con, P)
    _, dis_l = eng.topk_rows(-dist, P)
    rowptr = torch.arange(0, R + 1, 4, device=dev)
    rows = torch.arange(R, device=dev)
    launch = lambda: eng.blend_points(pref, rowptr, rows, I, points=P, weights=W, con=con_l, con_slot=con_slot, dis=dis_l,  # noqa: E731
                                      dis_slot=dis_slot, item_mask=mask, top=TOP)
    t_launch = timed(launch, args.reps)
    dense = lambda: torch_route(users_t, items_t, uid, number, con, dist, con_slot, dis_slot, mask)  # noqa: E731
    t_dense = timed(dense, args.reps)
    rating_t = dense().values
    same = bool(torch.equal(rating_t, rating_k))

    def loop(n):
        """demo.py:260-313 for the first n request rows, the live view only (one rating column per request column)"""
        rank2rate = torch.arange(P, 0, -1, device=dev, dtype=torch.float64)
        rating = torch.zeros((G, I), dtype=torch.float64, device=dev)
        all_rank = torch.topk(users_t[uid[:n]] @ items_t.T, P).indices
        for i in range(n):
            g = i // 4
            rating[g, all_rank[i]] += rank2rate * W[0]
            rating[g, torch.argsort(con[con_slot[i]])] += rank2rate * W[1]
            rating[g, torch.argsort(dist[dis_slot[i]])] += rank2rate * W[2]
        return rating

    n_loop = min(args.loop_rows, R)
    t_loop = timed(lambda: loop(n_loop), 1)[0]
med_call, med_launch, med_dense = (float(np.median(t)) for t in (t_call, t_launch, t_dense))
say(f"Seoul-shaped graph ({U} users x {I} items, embed 65 -> [64, 64]), R = {R} request rows in G = {G} columns, P = {P}, top {TOP}:")
say(f"  one recommend.blended_ranking call (propagation, rank_topk, 2 topk_rows, blend launch, 1 read-back): {fmt(t_call)}")
say(f"    of it the blend launch alone (engine.blend_points, lists given): {fmt(t_launch)}")
say(f"  torch ops on the same device (mm, topk, scatter_add_ into dense [G, n_item] tables, topk; tables given): {fmt(t_dense)}")
say(f"    ratings of the top lists equal bit for bit: {same}")
say(f"  per-row loop of the reference's shape on device tensors, {n_loop} rows: {t_loop:.1f} ms = {t_loop / n_loop * 1e3:.1f} us per row "
    f"-> {t_loop / n_loop * R:.0f} ms for {R} rows (scaled)")
say(f"  ratios: dense torch route / blended_ranking call = {med_dense / med_call:.2f}; dense torch route / blend launch = "
    f"{med_dense / med_launch:.2f}; per-row loop (scaled) / blended_ranking call = {t_loop / n_loop * R / med_call:.0f}")
if med_launch >= med_dense:
    say("  the blend launch is NOT faster than the dense torch route at 100 items; it stays: it is the only route at 100 K items")
del model

# ---- 2. C3-sized tables ------------------------------------------------------------------------------------------------------
if not args.skip_big:
    NU, NI, D = 1_000_000, 100_000, 512
    all_E = torch.randn((NU + NI, D), generator=gd, device=dev) * 0.1
    users_t, items_t = all_E[:NU], all_E[NU:]
    uid, number, con, dist, con_slot, dis_slot, mask = inputs(NU, NI, gd)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    state = {}

    def lists():
        state["pref"] = eng.rank_topk(users_t, items_t, P, user_ids=uid, status=status)[1]
        state["con"] = eng.topk_rows(-con, P)[1]
        state["dis"] = eng.topk_rows(-dist, P)[1]

    def blend():
        return eng.blend_points(state["pref"], rowptr, rows, NI, points=P, weights=W, con=state["con"], con_slot=con_slot,
                                dis=state["dis"], dis_slot=dis_slot, item_mask=mask, top=TOP, status=status)

    t_lists = timed(lists, args.reps)
    t_blend = timed(blend, args.reps)
    rating_k = blend()[1]
    assert int(status.item()) == 0
    say(f"C3-sized tables ({NU} users, {NI} items, D = {D}), R = {R} request rows in G = {G} columns, P = {P}, top {TOP}:")
    say(f"  rank_topk + 2 topk_rows: {fmt(t_lists)}")
    say(f"  blend launch (engine.blend_points, {(NI + 4095) // 4096} tiles of 4 096 items per column + merge): {fmt(t_blend)}")
    try:
        dense = lambda: torch_route(users_t, items_t, uid, number, con, dist, con_slot, dis_slot, mask, row_chunk=16384)  # noqa: E731
        t_dense = timed(dense, max(2, args.reps // 2))
        same = bool(torch.equal(dense().values, rating_k))
        med = float(np.median(t_lists)) + float(np.median(t_blend))
        say(f"  torch ops on the same device (scores in chunks of 16 384 rows, three dense [G, n_item] int64 tables = "
            f"{3 * G * NI * 8 / 1e9:.1f} GB + the fp64 ratings): {fmt(t_dense)}")
        say(f"    ratings of the top lists equal bit for bit: {same}")
        say(f"  ratio: dense torch route / (lists + blend launch) = {float(np.median(t_dense)) / med:.2f}")
    except torch.cuda.OutOfMemoryError as exc:
        say(f"  torch ops on the same device: out of memory ({str(exc)[:80]})")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
