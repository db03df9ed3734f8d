"""The per-group selection behind the train/test split (engine.select_per_group, csrc/select.hip) beside the torch-op formulation:
a `rand` key per row, a sort by (group, key), and a compare of every row's rank within its group with the group's quota.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  groups  --rows rows with 1, 100 and 100 000 groups (uniform draws), quota 30 % of every group: the selection alone, the LDS tier
          against the memory tier (option select_no_lds) wherever the LDS tier applies, and the torch-op formulation.
  seoul   a Seoul-shaped frame: --days x 100 destinations x 2 sexes x 8 ages rows with years 18 / 19 by date:
          preprocess.split_by_year and preprocess.split_stratified whole (counts, read-backs and nonzero included).
Per case: wall time of one call from columns already on the device, host clock around a synchronised call, median of --reps after
one warm-up.  Before anything is timed the mask is checked: exactly quota[g] rows per group, and the same mask from both tiers.
Writes its lines to --out (default profiles/split_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"groups": 600, "seoul": 300}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_lab.txt"))
ap.add_argument("--rows", type=int, default=50_000_000)
ap.add_argument("--days", type=int, default=730)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", choices=sorted(STEPS), help="run this step alone (the driver still starts it as a child)")
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the driver starts)")
args = ap.parse_args()

if args.step is None:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for step, limit in STEPS.items():
        if args.only and step != args.only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out, "--rows",
               str(args.rows), "--days", str(args.days), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from seoul_tourism_recommendation_ngcf_amd import _lib, engine as eng, preprocess  # noqa: E402

dev = torch.device("cuda:0")


def say(s):
    print(s, flush=True)
    with open(args.out, "a") as f:
        f.write(s + "\n")


def wall(fn, reps, warm=1):
    """ms per call, host clock, every call ended by a device synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def fmt(ms):
    return f"median {np.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}, {len(ms)} runs)"


def torch_select(group, quota_d, gen):
    """the torch-op formulation: a random key per row, rows sorted by (group, key), a row is taken iff its rank in its group is
    below the group's quota"""
    T = group.numel()
    key = torch.rand(T, device=group.device, generator=gen, dtype=torch.float64)
    by_key = torch.argsort(key)
    order = by_key[torch.sort(group[by_key], stable=True).indices]           # sorted by (group, key)
    sizes = torch.bincount(group, minlength=quota_d.numel())
    start = torch.cumsum(sizes, 0) - sizes
    g_sorted = group[order].long()
    rank = torch.arange(T, device=group.device) - start[g_sorted]
    mask = torch.zeros(T, dtype=torch.uint8, device=group.device)
    mask[order] = (rank < quota_d[g_sorted]).to(torch.uint8)
    return mask


def case(G, T, gen):
    group = torch.randint(0, G, (T,), device=dev, generator=gen, dtype=torch.int32)
    sizes = torch.bincount(group, minlength=G)
    quota = (sizes * 3 // 10).cpu()
    quota_d = quota.to(dev)
    lds_groups = eng.select_limits()[0]
    mask = eng.select_per_group(group, quota, seed=1)
    per_group = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, group.long(), mask.long())
    ok = torch.equal(per_group, quota_d)
    say(f"{T} rows, {G} groups, quota 30 % of every group ({int(quota.sum())} rows): exactly quota[g] rows per group: {ok}; "
        f"tier: {'LDS' if G <= lds_groups else 'memory'} (LDS up to {lds_groups} groups)")
    t_hip = wall(lambda: eng.select_per_group(group, quota, seed=1), args.reps)
    say(f"  engine.select_per_group:                                  {fmt(t_hip)}")
    if G <= lds_groups:
        _lib.set_option("select_no_lds", 1)
        same = torch.equal(mask, eng.select_per_group(group, quota, seed=1))
        t_mem = wall(lambda: eng.select_per_group(group, quota, seed=1), args.reps)
        _lib.set_option("select_no_lds", 0)
        say(f"  the same with select_no_lds = 1 (memory tier), same mask: {same}: {fmt(t_mem)}; memory / LDS = {np.median(t_mem) / np.median(t_hip):.2f}x")
    want = torch_select(group, quota_d, gen)
    ok = torch.equal(torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, group.long(), want.long()), quota_d)
    del want
    t_torch = wall(lambda: torch_select(group, quota_d, gen), args.reps)
    say(f"  torch ops (rand, sort by (group, key), rank compare; quotas met: {ok}): {fmt(t_torch)}; torch / HIP = {np.median(t_torch) / np.median(t_hip):.2f}x")


g = torch.Generator(device=dev).manual_seed(2604)
if args.step == "groups":
    for G in (1, 100, 100_000):
        case(G, args.rows, g)
else:
    n_dest = 100
    T = args.days * n_dest * 2 * 8
    t = torch.arange(T, device=dev)
    day_i = t // (n_dest * 16)
    year = torch.where(day_i < args.days // 2, 18, 19)
    dest = ((t // 16) % n_dest).to(torch.int32)
    say(f"Seoul-shaped frame: {T} rows, {int((year == 19).sum())} of year 19, {n_dest} destinations")
    tr, te = preprocess.split_by_year(year, seed=1)
    say(f"  split_by_year: {tr.numel()} train rows, {te.numel()} test rows: {fmt(wall(lambda: preprocess.split_by_year(year, seed=1), args.reps))}")
    tr, te = preprocess.split_stratified(dest, seed=1)
    say(f"  split_stratified: {tr.numel()} train rows, {te.numel()} test rows: {fmt(wall(lambda: preprocess.split_stratified(dest, seed=1), args.reps))}")
