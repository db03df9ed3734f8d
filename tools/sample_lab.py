"""Unseen-item draws on the device (engine.sample_unseen, sampling.train_triplets / test_candidates) against the host loop they replace
and against the same distribution from torch ops.

1. C3 graph (bench.py's 1 M users x 100 K items, ~50 M positives): an epoch of training triplets (m = 1 per positive row), and 1 M
   test cases at m = 24; set-up (ItemSets.from_pairs: a sort and unique) timed apart.
2. Seoul-shaped graph (graphs.seoul_standin: 5 840 users x 100 items, rows about 75 long): triplets for every positive row, candidate
   lists for the rows of users with at least 24 unseen items.
3. The comparisons.  The reference-shaped host loop (utils.py:234-262: np.setxor1d per user, np.random.choice per positive row) on the
   Seoul shape only, over --host-users users and scaled by rows.  Torch ops for m = 1 on both shapes: rejection sampling, the
   (user, item) keys looked up with searchsorted, redrawn until no row is rejected (one read-back per round).  Torch ops for m = 24 on
   the Seoul shape: random keys over the whole catalogue, seen items masked out, topk - a [T, n_item] matrix, which at 100 K items
   is not an option.

Writes its lines to --out (default profiles/sample_lab.txt) as well as to stdout."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_lab.txt"))
ap.add_argument("--interactions", type=int, default=50_000_000)
ap.add_argument("--test-cases", type=int, default=1_000_000)
ap.add_argument("--host-users", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
eng = pkg.engine
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


def torch_one(users, keys, n_item, gen):
    """One unseen item per row from torch ops: draw, look the (user, item) key up in the sorted keys, redraw the rejected rows."""
    neg = torch.randint(0, n_item, users.shape, generator=gen, device=users.device)
    todo = torch.arange(users.numel(), device=users.device)
    while True:
        k = users[todo] * n_item + neg[todo]
        pos = torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)
        todo = todo[keys[pos] == k]
        if int(todo.numel()) == 0:                # the round's read-back
            return neg
        neg[todo] = torch.randint(0, n_item, todo.shape, generator=gen, device=users.device)


def device_side(name, users, items, n_user, n_item, cases_m24):
    say(f"{name}: {n_user} users x {n_item} items, {int(users.numel())} positive rows")
    t0 = time.perf_counter()
    seen = eng.ItemSets.from_pairs(users, items, n_user, n_item)
    torch.cuda.synchronize()
    say(f"  set-up, ItemSets.from_pairs (sort + unique, once per data set): {(time.perf_counter() - t0) * 1e3:.1f} ms wall (first call)")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out1 = torch.empty((int(users.numel()), 1), dtype=torch.int64, device=dev)
    t1 = timed(lambda: eng.sample_unseen(seen, users, 1, 2024, out=out1, status=status), args.reps)
    say(f"  an epoch of triplets, m = 1 per positive row (engine.sample_unseen into a caller's buffer): {fmt(t1)} = "
        f"{int(users.numel()) / np.median(t1) / 1e6:.2f} G rows/s")
    api = timed(lambda: pkg.sampling.train_triplets(users, items, seen, seed=2024, n_user=n_user, n_item=n_item), args.reps)
    say(f"  the same through sampling.train_triplets (allocates, reads the status word back): {fmt(api)}")
    uid, first = cases_m24
    out24 = torch.empty((int(uid.numel()), 25), dtype=torch.int64, device=dev)
    t24 = timed(lambda: eng.sample_unseen(seen, uid, 24, 2024, first=first, out=out24, status=status), args.reps)
    say(f"  {int(uid.numel())} test cases, m = 24 + the held-out column: {fmt(t24)} = {int(uid.numel()) / np.median(t24) / 1e3:.1f} M cases/s")
    assert int(status.item()) == 0, int(status.item())
    keys = users * n_item + items                  # sorted and unique: synthetic_interactions / the Laplacian's row order
    gen = torch.Generator(device=dev).manual_seed(1)
    tt = timed(lambda: torch_one(users, keys, n_item, gen), max(2, args.reps // 2))
    say(f"  torch ops, m = 1 (rejection sampling, searchsorted on the pair keys, a read-back per round): {fmt(tt)} = "
        f"{np.median(tt) / np.median(t1):.1f}x the kernel")
    return seen, float(np.median(t1)), float(np.median(t24))


# ---- 1. C3 -----------------------------------------------------------------------------------------------------------------------
NU, NI = 1_000_000, 100_000
u, i, _ = pkg.graphs.synthetic_interactions(NU, NI, args.interactions, seed=2603, device=dev)
gd = torch.Generator(device=dev).manual_seed(3)
pick = torch.randint(0, int(u.numel()), (args.test_cases,), generator=gd, device=dev)
device_side("C3 graph", u, i, NU, NI, (u[pick].contiguous(), i[pick].contiguous()))
del u, i, pick

# ---- 2. Seoul shape ----------------------------------------------------------------------------------------------------------------
coo = pkg.graphs.seoul_standin(dev)[0]
SU, SI = coo["n_user"], coo["n_item"]
sel = coo["rows"] < SU
su, si = coo["rows"][sel].to(torch.int64), (coo["cols"][sel] - SU).to(torch.int64)
order = torch.argsort(su * SI + si)
su, si = su[order].contiguous(), si[order].contiguous()
deg = torch.bincount(su, minlength=SU)
roomy = deg[su] <= SI - 24                         # rows of users with at least 24 unseen items
say(f"Seoul-shaped graph: seen rows of {float(deg.double().mean()):.1f} items on average (max {int(deg.max())}); "
    f"{int(roomy.sum())} of {int(su.numel())} rows belong to users with >= 24 unseen items")
_, s1, s24 = device_side("Seoul-shaped graph", su, si, SU, SI, (su[roomy].contiguous(), si[roomy].contiguous()))

# torch ops for m = 24 on 100 items: random keys, seen items pushed to the end, the 24 smallest
tu = su[roomy]
seen_mask = torch.zeros((SU, SI), dtype=torch.bool, device=dev)
seen_mask[su, si] = True
gen = torch.Generator(device=dev).manual_seed(2)


def torch_24():
    keys = torch.rand((int(tu.numel()), SI), generator=gen, device=dev)
    keys[seen_mask[tu]] = 2.0
    return torch.topk(keys, 24, dim=1, largest=False).indices


tm = timed(torch_24, args.reps)
say(f"  torch ops, m = 24 (a [T, {SI}] matrix of random keys, seen items masked, topk): {fmt(tm)} = {np.median(tm) / s24:.1f}x the kernel")

# ---- 3. the reference-shaped host loop, Seoul shape --------------------------------------------------------------------------------
hu, hi = su.cpu().numpy(), si.cpu().numpy()
all_items = np.arange(SI)
bounds = np.searchsorted(hu, np.arange(args.host_users + 1))
np.random.seed(0)
for m in (1, 24):
    rows, t0 = 0, time.perf_counter()
    for user in range(args.host_users):
        pos_items = hi[bounds[user]:bounds[user + 1]]
        neg_items = np.setxor1d(all_items, pos_items)
        if len(neg_items) < m:
            continue
        for _ in pos_items:
            np.random.choice(neg_items.copy(), m, replace=False)
            rows += 1
    dt = (time.perf_counter() - t0) * 1e3
    total = int(su.numel()) if m == 1 else int(roomy.sum())
    est = dt / max(rows, 1) * total
    say(f"  reference-shaped host loop, m = {m} (setxor1d per user, np.random.choice per row): {dt:.0f} ms for {rows} rows of "
        f"{args.host_users} users = {dt / max(rows, 1) * 1e3:.1f} us per row; scaled to {total} rows {est:.0f} ms = "
        f"{est / (s1 if m == 1 else s24):.0f}x the kernel")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
