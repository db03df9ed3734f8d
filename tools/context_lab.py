"""The trip context of a recommendation request (csrc/context.hip) beside its yardsticks: the float pivot against `index_add_` (torch
ops; DIFFERENT BITS - a plain atomic sum in arrival order, not pandas' compensated one) and against pandas on the host, and the
distance table against numpy.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  c3      --rows raw rows with C3's cardinalities (365 days x 100 K items, uniform draws): engine.context.group_sum_float of one
          float64 column over (month, day, dayofweek, item), whole and split into group_by / segments_from_ids / the Kahan kernel,
          for every `wave_min` of --wave-min (0 = the library's default).
  seoul   the Seoul-shaped log, one row per hour, day and item (24 x 365 x 100), in file order and shuffled, also against pandas.
  giant   one group of --giant rows and nothing else: the wave tier's chain alone, against the lane tier on the same rows.
  dist    recommend.distance_table for 424 departure points x 100 K items against the same formula in numpy on the host.
Per case: wall time of one call from columns already on the device, host clock around a synchronised call, median of --reps after
one warm-up.  The Kahan sums are compared across all `wave_min` (they must be bit-equal) before anything is timed.
Writes its lines to --out (default profiles/context_lab.txt) as well as to stdout."""
import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"c3": 600, "seoul": 420, "giant": 300, "dist": 300}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_lab.txt"))
ap.add_argument("--rows", type=int, default=50_000_000)
ap.add_argument("--giant", type=int, default=8_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--wave-min", default="0,16,64,256,1024,4096")
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
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out, "--rows",
               str(args.rows), "--giant", str(args.giant), "--reps", str(args.reps), "--wave-min", args.wave_min]
        rc = subprocess.run(cmd + (["--no-pandas"] if args.no_pandas else [])).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from seoul_tourism_recommendation_ngcf_amd import engine as eng, recommend  # noqa: E402

WAVE_MIN = [int(x) for x in args.wave_min.split(",")]
dev = torch.device("cuda:0")
ctx = eng.context


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


def bits(t):
    return t.view(torch.int64)


def pivot_case(name, columns, value, pandas_too=False):
    T = int(value.numel())
    groups = eng.group_by(columns, inverse=True)
    G = int(groups.keys[0].numel())
    rowptr, order = eng.segments_from_ids(groups.inverse, G)
    longest = int((rowptr[1:] - rowptr[:-1]).max())
    first = ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=WAVE_MIN[0])[0]
    same = all(torch.equal(bits(first), bits(ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=w)[0])) for w in WAVE_MIN[1:])
    plain = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, groups.inverse, value)
    say(f"{name}: {T} rows, {G} groups, longest {longest} rows; Kahan sums bit-equal across wave_min {WAVE_MIN}: {same}; groups whose "
        f"index_add_ sum has other bits: {int((bits(plain) != bits(first)).sum())}")
    t = wall(lambda: torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, groups.inverse, value), args.reps)
    say(f"  index_add_ on the group index (DIFFERENT BITS: atomic adds in arrival order, no compensation): {fmt(t)}")
    say(f"  engine.group_by(inverse=True), the keys and the group index:   {fmt(wall(lambda: eng.group_by(columns, inverse=True), args.reps))}")
    say(f"  engine.segments_from_ids, the stable order (a library sort):    {fmt(wall(lambda: eng.segments_from_ids(groups.inverse, G), args.reps))}")
    best = None
    for w in WAVE_MIN:
        t = wall(lambda: ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=w), args.reps)
        say(f"  engine.context.segment_kahan_sum, wave_min={w:5d}:               {fmt(t)}")
        if best is None or np.median(t) < best[1]:
            best = (w, float(np.median(t)))
    say(f"  fastest wave_min here: {best[0]} (0 is the library's default)")
    say(f"  engine.context.group_sum_float, the whole pivot:                {fmt(wall(lambda: ctx.group_sum_float(columns, value), args.reps))}")
    if pandas_too and not args.no_pandas:
        import pandas as pd
        names = ["month", "day", "dayofweek", "destination"]
        df = pd.DataFrame({n: c.cpu().numpy() for n, c in zip(names, columns)})
        df["congestion_1"] = value.cpu().numpy()
        t0 = time.perf_counter()
        pv = pd.pivot_table(df, index=names, aggfunc={"congestion_1": "sum"}).reset_index()
        ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(pv["congestion_1"].values.view(np.int64), first.cpu().numpy().view(np.int64))
        say(f"  pandas pivot_table on the host (one run): {ms:.0f} ms, {len(pv)} rows; its sums bit-equal to the device's: {same}")


def calendar(day_index):
    """(month, day, dayofweek) int32 columns of day-of-year indices 0 .. 364 (no leap year, the year starts on a Tuesday)"""
    starts = torch.tensor(np.cumsum((0,) + recommend.MONTH_DAYS), device=dev)
    month = torch.bucketize(day_index, starts, right=True)
    return month.to(torch.int32), (day_index - starts[month - 1] + 1).to(torch.int32), ((day_index + 1) % 7).to(torch.int32)


g = torch.Generator(device=dev).manual_seed(2611)
if args.step == "c3":
    T, n_item = args.rows, 100_000
    month, day, dow = calendar(torch.randint(0, 365, (T,), device=dev, generator=g))
    item = torch.randint(0, n_item, (T,), device=dev, generator=g, dtype=torch.int32)
    value = torch.rand(T, device=dev, generator=g, dtype=torch.float64) * 100
    pivot_case("C3 cardinalities: 365 days x 100 K items, uniform draws", [month, day, dow, item], value)
elif args.step == "seoul":
    n_item, hours = 100, 24
    t = torch.arange(365 * n_item * hours, device=dev)                 # file order: day, item, hour
    month, day, dow = calendar(t // (n_item * hours))
    item = ((t // hours) % n_item).to(torch.int32)
    value = torch.rand(int(t.numel()), device=dev, generator=g, dtype=torch.float64) * 100
    pivot_case("Seoul-shaped log, file order", [month, day, dow, item], value)
    perm = torch.randperm(int(t.numel()), device=dev, generator=g)
    pivot_case("Seoul-shaped log, shuffled", [c[perm].contiguous() for c in (month, day, dow, item)], value[perm].contiguous(), pandas_too=True)
elif args.step == "giant":
    T = args.giant
    value = torch.rand(T, device=dev, generator=g, dtype=torch.float64) * 100
    rowptr = torch.tensor([0, T], device=dev)
    order = torch.randperm(T, device=dev, generator=g).sort().values  # the identity, read through `order` as the pivot does
    a = ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=1)[0]
    b = ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=T + 1)[0]
    say(f"one group of {T} rows: wave tier and lane tier bit-equal: {torch.equal(bits(a), bits(b))}")
    t = wall(lambda: ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=1), args.reps)
    say(f"  wave tier (wave_min=1):      {fmt(t)}; {np.median(t) * 1e3 / (T / 64):.3f} us per 64 rows")
    t = wall(lambda: ctx.segment_kahan_sum(rowptr, value, order=order, wave_min=T + 1), max(args.reps // 2, 1))
    say(f"  lane tier (wave_min=T + 1):  {fmt(t)}; {np.median(t) * 1e3 / (T / 64):.3f} us per 64 rows")
else:
    S, n_item = 424, 100_000
    dep = torch.stack([torch.rand(S, device=dev, generator=g, dtype=torch.float64) * 0.3 + 37.4,
                       torch.rand(S, device=dev, generator=g, dtype=torch.float64) * 0.4 + 126.8], 1)
    item = torch.stack([torch.rand(n_item, device=dev, generator=g, dtype=torch.float64) * 0.3 + 37.4,
                        torch.rand(n_item, device=dev, generator=g, dtype=torch.float64) * 0.4 + 126.8], 1)
    out = torch.empty((S, n_item), dtype=torch.float64, device=dev)
    t = wall(lambda: ctx.haversine_table(dep, item, out=out), args.reps)
    say(f"distance table, {S} departure points x {n_item} items (Seoul box): engine.context.haversine_table {fmt(t)}; "
        f"{S * n_item * 8 / np.median(t) / 1e6:.1f} GB/s of output")
    d, it = dep.cpu().numpy(), item.cpu().numpy()

    def host():
        k = math.pi / 180
        lat1, lng1, lat2, lng2 = (d[:, 0] * k)[:, None], (d[:, 1] * k)[:, None], (it[:, 0] * k)[None, :], (it[:, 1] * k)[None, :]
        a, b = np.sin((lat2 - lat1) * 0.5), np.sin((lng2 - lng1) * 0.5)
        return ((2 * 6371.0088) * np.arcsin(np.sqrt(a * a + (np.cos(lat1) * np.cos(lat2)) * (b * b)))) * 1000

    t0 = time.perf_counter()
    want = host()
    ms = (time.perf_counter() - t0) * 1e3
    err = np.abs(out.cpu().numpy() - want) / np.spacing(want)
    say(f"  the same formula in numpy on the host (one run): {ms:.0f} ms; device against it: max {err.max():.1f} ulp")
