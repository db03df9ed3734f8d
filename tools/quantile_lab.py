"""The per-user quartile floor on the device (preprocess.scale_implicit, engine.segment_quantile_floor) against the same result
from torch ops and against the reference's pandas loop.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  c3      C3 shape (bench.py's 1 M users, --rows = 50 M rows of integer counts): set-up (segments_from_ids, standard_stats) timed apart,
          then the kernel at wave_max = 64 (the default), 32, 16 and 1 (everything on the workgroup tier), with `order` and
          pre-grouped; then the torch-ops baseline: a stable sort by value, then by user, the two order statistics by indexing.
  seoul   Seoul-shaped stand-in (graphs.seoul_standin: 5 840 users, rows about 75 long per year slice): the same two.
  pandas  the reference-shaped loop (utils.py:117-121: isin -> quantile(q=0.25) -> masked write) on the Seoul shape, host only,
          over --host-users users and scaled by users.
Every device result is checked against the torch-ops result bit for bit before it is timed.
Writes its lines to --out (default profiles/quantile_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"c3": 600, "seoul": 180, "pandas": 300}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_lab.txt"))
ap.add_argument("--rows", type=int, default=50_000_000)
ap.add_argument("--host-users", type=int, default=300)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the driver starts)")
args = ap.parse_args()

if args.step is None:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for step, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out,
               "--rows", str(args.rows), "--host-users", str(args.host_users), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

eng, pre = pkg.engine, pkg.preprocess


def say(s):
    print(s, flush=True)
    with open(args.out, "a") as f:
        f.write(s + "\n")


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


def torch_floor(users, x, n_user, mean, scale, shift):
    """The same result from torch ops: rows sorted by (user, value), the two order statistics by indexing, the blend written as the
    kernel's header states it."""
    z = ((x - mean) / scale) + shift
    by_value = torch.sort(z, stable=True)
    by_user = torch.sort(users[by_value.indices], stable=True)
    zs = by_value.values[by_user.indices]
    n = torch.bincount(users, minlength=n_user)
    start = torch.cumsum(n, 0) - n
    r = (n - 1).clamp_(min=0)
    lo, t = r // 4, (r % 4).double() * 0.25
    last = (zs.numel() - 1) if zs.numel() else 0
    a = zs[(start + lo).clamp_(max=last)]
    b = zs[(start + torch.minimum(lo + 1, r)).clamp_(max=last)]
    quant = torch.where(t < 0.5, a + (b - a) * t, b - (b - a) * (1 - t))
    quant = torch.where(n > 0, quant, torch.full_like(quant, float("nan")))
    return torch.where(z < quant[users], torch.zeros_like(z), z), quant


def device_side(name, users, counts, n_user):
    T = int(users.numel())
    say(f"{name}: {n_user} users, {T} rows, {T / n_user:.1f} per user")
    t0 = time.perf_counter()
    rowptr, order = eng.segments_from_ids(users, n_user)
    torch.cuda.synchronize()
    say(f"  set-up, segments_from_ids (a stable sort, bincount, cumsum): {(time.perf_counter() - t0) * 1e3:.1f} ms wall (first call)")
    t0 = time.perf_counter()
    mean, scale, shift = pre.standard_stats(counts)
    say(f"  set-up, standard_stats (fp64 reductions, three read-backs): {(time.perf_counter() - t0) * 1e3:.1f} ms wall (first call)")
    lens = rowptr.diff()
    say(f"  segment lengths: max {int(lens.max())}, {int((lens > 64).sum())} longer than 64, {int((lens > 2048).sum())} longer than 2048")
    x = counts.to(torch.float64)
    want, want_q = torch_floor(users, x, n_user, mean, scale, shift)
    out, quant = torch.empty_like(x), torch.empty(n_user, dtype=torch.float64, device=x.device)
    status = torch.zeros(1, dtype=torch.int32, device=x.device)
    xg = x[order].contiguous()
    base = None
    for wave_max in (64, 32, 16, 1):
        def run(wm=wave_max):
            return eng.segment_quantile_floor(rowptr, x, order=order, mean=mean, scale=scale, shift=shift, wave_max=wm, out=out, quant=quant,
                                              status=status)
        run()
        ok = torch.equal(out, want) and torch.equal(quant.nan_to_num(nan=-1.0), want_q.nan_to_num(nan=-1.0)) and int(status.item()) == 0
        ms = timed(run, args.reps)
        base = base or float(np.median(ms))
        say(f"  kernel through `order`, wave_max = {wave_max}: {fmt(ms)} = {T / np.median(ms) / 1e6:.2f} G rows/s; equals torch ops: {ok}")
    ms = timed(lambda: eng.segment_quantile_floor(rowptr, xg, mean=mean, scale=scale, shift=shift, out=out, quant=quant, status=status),
               args.reps)
    say(f"  kernel on pre-grouped rows (order = None): {fmt(ms)}")
    ms = timed(lambda: pre.scale_implicit(users, counts, n_user=n_user, stats=(mean, scale, shift)), max(2, args.reps // 2))
    say(f"  preprocess.scale_implicit with stats given (set-up + kernel + status read-back): {fmt(ms)}")
    ms = timed(lambda: torch_floor(users, x, n_user, mean, scale, shift), max(2, args.reps // 2))
    say(f"  torch ops (two stable sorts + indexing): {fmt(ms)} = {np.median(ms) / base:.1f}x the kernel at wave_max = 64")


def seoul_rows(device):
    coo = pkg.graphs.seoul_standin(device)[0]
    sel = coo["rows"] < coo["n_user"]
    users = coo["rows"][sel].to(torch.int64).contiguous()
    g = torch.Generator(device="cpu").manual_seed(5)
    counts = torch.randint(0, 50, (int(users.numel()),), generator=g)
    counts[torch.rand(counts.shape, generator=g) < 0.02] *= 1000
    return users, counts.to(users.device), int(coo["n_user"])


if args.step == "c3":
    dev = torch.device("cuda:0")
    NU = 1_000_000
    g = torch.Generator(device=dev).manual_seed(2603)
    users = torch.randint(0, NU, (args.rows,), generator=g, device=dev)
    counts = torch.randint(0, 50, (args.rows,), generator=g, device=dev)
    counts[torch.rand(args.rows, generator=g, device=dev) < 0.02] *= 1000
    device_side("C3 shape", users, counts, NU)
elif args.step == "seoul":
    device_side("Seoul-shaped stand-in", *seoul_rows(torch.device("cuda:0")))
else:
    import pandas as pd
    users, counts, n_user = seoul_rows("cpu")
    df = pd.DataFrame({"userid": users.numpy(), "rating": counts.double().numpy()})
    df["rating"] = (df["rating"] - df["rating"].mean()) / df["rating"].std(ddof=0)
    df["rating"] = df["rating"] + np.abs(df["rating"].min())
    t0 = time.perf_counter()
    for userid in df["userid"].unique()[:args.host_users]:
        tmp = df.loc[df["userid"].isin([userid])]
        quarter = tmp["rating"].quantile(q=0.25)
        neg_tmp = tmp.loc[tmp["rating"] < quarter]
        df.loc[neg_tmp.index, "rating"] = 0
    dt = (time.perf_counter() - t0) * 1e3
    done = min(args.host_users, n_user)
    say(f"reference-shaped pandas loop, Seoul shape ({len(df)} rows): {dt:.0f} ms for {done} users = {dt / done:.2f} ms per user; "
        f"scaled to {n_user} users {dt / done * n_user:.0f} ms")
