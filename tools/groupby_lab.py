"""The pivot and the two id maps of the reference's first stage (engine.group_by, csrc/groupby.hip) beside the torch-op formulation
(`torch.unique(dim=0, return_inverse=True)` plus `index_add_`, which sorts the whole table) and, on the Seoul shape, pandas.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  seoul   a Seoul-shaped raw table: --days x 100 destinations x 2 sexes x 8 ages x 24 time-zone rows, in file order and shuffled:
          the pivot over (date, destination, dayofweek, sex, age), then both id maps over the pivoted rows.
  c3      --rows rows with C3's cardinalities (1 M users x 100 K items, uniform draws): group_by((user, item), (count,)) and the
          inverse map of the users.
Per case: wall time of one call from columns already on the device, host clock around a synchronised call, median of --reps after
one warm-up, for every `lds_slots` of --lds (0 = the LDS stage off); the results are compared with the torch-op result before
anything is timed.  The fastest `lds_slots` per case is named; engine.GROUPBY_LDS_SLOTS is the default the package ships.
Writes its lines to --out (default profiles/groupby_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"seoul": 420, "c3": 900}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_lab.txt"))
ap.add_argument("--days", type=int, default=730)
ap.add_argument("--rows", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lds", default="0,64,256,1024,2048")
ap.add_argument("--no-pandas", action="store_true")
ap.add_argument("--only", choices=sorted(STEPS), help="run this step alone (the driver still starts it as a child)")
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the driver starts)")
args = ap.parse_args()

if args.step is None:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for step, limit in STEPS.items():
        if args.only and step != args.only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out, "--days",
               str(args.days), "--rows", str(args.rows), "--reps", str(args.reps), "--lds", args.lds] + (["--no-pandas"] if args.no_pandas else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from seoul_tourism_recommendation_ngcf_amd import engine as eng, preprocess  # noqa: E402

LDS = [int(x) for x in args.lds.split(",")]
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


def torch_group_by(columns, values, inverse):
    """the torch-op formulation: unique rows (a sort of the whole table) plus index_add_"""
    uniq, inv = torch.unique(torch.stack([c.to(torch.int64) for c in columns], 1), dim=0, return_inverse=True)
    sums = [torch.zeros(uniq.shape[0], dtype=torch.int64, device=inv.device).index_add_(0, inv, v.to(torch.int64)) for v in values]
    return uniq, sums, inv if inverse else None


def case(name, columns, values, inverse):
    T = int(columns[0].numel())
    want = torch_group_by(columns, values, inverse)
    got = eng.group_by(columns, values, inverse=inverse)
    same = all(torch.equal(k, want[0][:, j]) for j, k in enumerate(got.keys)) and all(torch.equal(a, b) for a, b in zip(got.sums, want[1]))
    same = same and (not inverse or torch.equal(got.inverse, want[2]))
    say(f"{name}: {T} rows, {len(columns)} key columns, {len(values)} value columns, inverse={inverse}: {int(got.keys[0].numel())} groups; "
        f"equal to the torch-op result: {same}")
    del want, got
    t_torch = wall(lambda: torch_group_by(columns, values, inverse), args.reps)
    say(f"  torch.unique(dim=0) + index_add_ (the yardstick): {fmt(t_torch)}")
    best = None
    for lds in LDS:
        t = wall(lambda: eng.group_by(columns, values, inverse=inverse, lds_slots=lds), args.reps)
        say(f"  engine.group_by, lds_slots={lds:5d}:                  {fmt(t)}; torch / HIP = {np.median(t_torch) / np.median(t):.2f}x")
        if best is None or np.median(t) < best[1]:
            best = (lds, float(np.median(t)))
    say(f"  fastest lds_slots here: {best[0]} (shipped default: {eng.GROUPBY_LDS_SLOTS})")
    return best[0]


g = torch.Generator(device=dev).manual_seed(2603)
if args.step == "seoul":
    n_dest, zones = 100, 24
    first = np.datetime64("2018-01-01")
    days = first + np.arange(args.days)
    ymd = torch.tensor([int(str(d).replace("-", "")) for d in days], dtype=torch.int64, device=dev)
    dow_of = torch.tensor([(int((d - np.datetime64("1970-01-05")).astype(int)) % 7) for d in days], dtype=torch.int64, device=dev)
    dest_codes = torch.sort(torch.randperm(2_400_000, device=dev, generator=g)[:n_dest] + 125_452).values
    ages = torch.arange(5, 85, 10, device=dev)
    T = args.days * n_dest * 2 * 8 * zones
    t = torch.arange(T, device=dev)                                   # file order: day, destination, time zone, sex, age
    age, r = ages[t % 8], t // 8
    sex, r = r % 2, r // 2
    r = r // zones
    dest, day_i = dest_codes[r % n_dest], r // n_dest
    date, dow = ymd[day_i], dow_of[day_i]
    visitor = torch.randint(0, 500, (T,), device=dev, generator=g)
    del t, r, day_i
    cols = [date, dest, dow.to(torch.int32), sex.to(torch.int32), age.to(torch.int32)]
    chosen = []
    for order in ("file order", "shuffled"):
        if order == "shuffled":
            perm = torch.randperm(T, device=dev, generator=g)
            cols, visitor = [c[perm].contiguous() for c in cols], visitor[perm].contiguous()
            del perm
        chosen.append(case(f"Seoul-shaped raw table, {order}: the pivot", cols, [visitor], False))
        chosen.append(case(f"Seoul-shaped raw table, {order}: destinations alone (100 groups, every row on them)", cols[1:2], [visitor], True))
    if not args.no_pandas:
        import pandas as pd
        names = ["date", "destination", "dayofweek", "sex", "age"]
        df = pd.DataFrame({n: c.cpu().numpy() for n, c in zip(names, cols)})
        df["visitor"] = visitor.cpu().numpy()
        t0 = time.perf_counter()
        pv = pd.pivot_table(df, index=names, aggfunc={"visitor": "sum"}).reset_index()
        say(f"  pandas pivot_table of the shuffled table on the host (one run, integer dates): {(time.perf_counter() - t0) * 1e3:.0f} ms, {len(pv)} rows")
        del df, pv
    table = preprocess.aggregate_visits(*cols, visitor)
    say(f"pivoted rows: {len(table)}")
    code = eng.decimal_code((table.age, table.sex, table.month, table.day), preprocess.USER_KEY_WIDTHS)
    t_code = wall(lambda: eng.decimal_code((table.age, table.sex, table.month, table.day), preprocess.USER_KEY_WIDTHS), args.reps)
    say(f"  engine.decimal_code of the pivoted rows: {fmt(t_code)}")
    chosen.append(case("user map of the pivoted rows (string order through the base-11 code)", [code], [], True))
    chosen.append(case("item map of the pivoted rows", [table.destination], [], True))
    t_map = wall(lambda: preprocess.map_ids(table.age, table.sex, table.month, table.day, table.destination), args.reps)
    say(f"  preprocess.map_ids, both maps: {fmt(t_map)}")
    say(f"fastest lds_slots per case of this step: {chosen}")
else:
    n_user, n_item, T = 1_000_000, 100_000, args.rows
    user = torch.randint(0, n_user, (T,), device=dev, generator=g, dtype=torch.int32)
    item = torch.randint(0, n_item, (T,), device=dev, generator=g, dtype=torch.int32)
    count = torch.randint(0, 9, (T,), device=dev, generator=g, dtype=torch.int32)
    chosen = [case("C3 cardinalities: (user, item) pairs, nearly all distinct", [user, item], [count], False),
              case("C3 cardinalities: users alone, with the inverse", [user], [count], True)]
    say(f"fastest lds_slots per case of this step: {chosen}")
