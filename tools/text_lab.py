"""Reading the raw visit log on the device (csrc/text.hip) beside its yardsticks: `pd.read_csv(usecols=...)` on the host, and
`np.loadtxt` on a sample.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  seoul   a Seoul-shaped log (--seoul-rows lines, the reference's nine column names, fixed-width zero-padded integer fields, 43 bytes
          per line), generated on the device: `preprocess.read_visits` from the bytes on the device, and split into its passes -
          count, cumsum, starts, parse - with bytes/s for each; the parse on the LDS tier and on the memory tier (`tier=`); the
          whole against `pd.read_csv(io.BytesIO(...), sep='|', usecols=...)` and against `np.loadtxt` on the first --sample lines.
  c3      --rows lines with C3's cardinalities (365 days x 100 K destinations): the same passes, no host yardstick.
  floats  --float-rows lines of three float columns, 15 digits each (fast fields) and 19 digits each (slow fields: the host patch).
Per case: wall time of one call, host clock around a synchronised call, median of --reps after one warm-up.  The columns of the
two tiers are compared (they must be bit-equal) before anything is timed.
Writes its lines to --out (default profiles/text_lab.txt) as well as to stdout."""
import argparse
import io
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"seoul": 900, "c3": 600, "floats": 300}                         # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_lab.txt"))
ap.add_argument("--seoul-rows", type=int, default=28_000_000)
ap.add_argument("--rows", type=int, default=200_000_000)
ap.add_argument("--float-rows", type=int, default=20_000_000)
ap.add_argument("--sample", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
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
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out, "--seoul-rows",
               str(args.seoul_rows), "--rows", str(args.rows), "--float-rows", str(args.float_rows), "--sample", str(args.sample), "--reps",
               str(args.reps)]
        rc = subprocess.run(cmd + (["--no-pandas"] if args.no_pandas else [])).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from seoul_tourism_recommendation_ngcf_amd import engine as eng, preprocess  # noqa: E402

dev = torch.device("cuda:0")
text = eng.text
HEADER = ("date", "date365", "dayofweek", "area", "destination", "sex", "age", "visitor", "total_num")
WIDTHS = (8, 3, 1, 2, 6, 1, 2, 5, 6)
KEYS = list(preprocess.VISIT_COLUMNS)


def say(line: str):
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def fixed_width(columns, widths, chunk=4_000_000):
    """uint8 text of zero-padded integer columns, '|' between them and '\\n' after each line, built on the device chunk by chunk."""
    T, line = int(columns[0].numel()), sum(widths) + len(widths)
    out = torch.empty(T * line, dtype=torch.uint8, device=dev)
    for lo in range(0, T, chunk):
        hi = min(lo + chunk, T)
        rows = out[lo * line:hi * line].view(hi - lo, line)
        at = 0
        for col, w in zip(columns, widths):
            for k in range(w):
                rows[:, at + k] = ((col[lo:hi] // 10 ** (w - 1 - k)) % 10 + 48).to(torch.uint8)
            rows[:, at + w] = ord("|")
            at += w + 1
        rows[:, line - 1] = ord("\n")
    return out


def visit_log(T, n_dest, n_days, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda hi: torch.randint(0, hi, (T,), device=dev, generator=g)   # noqa: E731
    day = r(n_days)
    date = torch.where(day < n_days // 2, 20180101, 20190101) + (day % (n_days // 2)) % 28 + 100 * ((day % (n_days // 2)) // 28)
    cols = (date, day % 365 + 1, day % 7, r(25) + 1, r(n_dest) + 100000, r(2), 5 * r(16), r(5000), r(100000))
    head = torch.tensor(list(("|".join(HEADER) + "\n").encode()), dtype=torch.uint8, device=dev)
    return torch.cat([head, fixed_width(cols, WIDTHS)])


def passes(data, name, fields, kinds, n_fields):
    """The passes of read_table one by one, and the two tiers of the parse."""
    lib, n = eng._lib.load(), int(data.numel())
    status = text._new_status(dev)
    block = text.limits()[2]
    counts = torch.empty((n + block - 1) // block, dtype=torch.int64, device=dev)
    t = timed(lambda: eng._lib.check(lib.ngcf_text_count_rows(eng._ptr(data), n, eng._ptr(counts), eng._ptr(status), eng._stream())))
    say(f"{name}: count pass             {t * 1e3:9.3f} ms  {n / t / 1e9:8.2f} GB/s")
    t = timed(lambda: torch.cumsum(counts, 0))
    say(f"{name}: cumsum of {counts.numel()} blocks  {t * 1e3:9.3f} ms")
    t = timed(lambda: text.row_starts(data))
    say(f"{name}: row_starts (both passes, cumsum, read-back) {t * 1e3:9.3f} ms  {n / t / 1e9:8.2f} GB/s")
    starts = text.row_starts(data)
    cols = {tier: text.parse_columns(data, starts, fields, kinds, n_fields=n_fields, skip_rows=1, tier=tier) for tier in ("lds", "memory")}
    same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(cols["lds"], cols["memory"]))
    say(f"{name}: {int(starts.numel()) - 2} rows; LDS tier and memory tier bit-equal: {same}")
    del cols
    for tier in ("lds", "memory"):
        t = timed(lambda: text.parse_columns(data, starts, fields, kinds, n_fields=n_fields, skip_rows=1, tier=tier))
        say(f"{name}: parse, tier {tier:6s}       {t * 1e3:9.3f} ms  {n / t / 1e9:8.2f} GB/s")


def visits(step, T, n_dest, n_days, host):
    data = visit_log(T, n_dest, n_days, 1)
    say(f"{step}: {T} lines, {int(data.numel())} bytes, limits {text.limits()}")
    passes(data, step, [HEADER.index(c) for c in KEYS], [0] * len(KEYS), len(HEADER))
    t = timed(lambda: preprocess.read_visits(data))
    say(f"{step}: preprocess.read_visits   {t * 1e3:9.3f} ms  {int(data.numel()) / t / 1e9:8.2f} GB/s")
    t = timed(lambda: preprocess.load_visits(data))
    say(f"{step}: preprocess.load_visits   {t * 1e3:9.3f} ms")
    if not host:
        return
    raw = data.cpu().numpy().tobytes()
    t0 = time.perf_counter()
    dev_copy = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    say(f"{step}: host to device copy      {(time.perf_counter() - t0) * 1e3:9.3f} ms")
    del dev_copy
    if not args.no_pandas:
        import pandas as pd
        t0 = time.perf_counter()
        df = pd.read_csv(io.BytesIO(raw), sep="|", usecols=KEYS)
        say(f"{step}: pd.read_csv(usecols=)    {(time.perf_counter() - t0) * 1e3:9.3f} ms (host, once)")
        got = preprocess.read_visits(data)
        say(f"{step}: equal to pandas: {all(np.array_equal(g.cpu().numpy(), df[c].to_numpy()) for g, c in zip(got, KEYS))}")
    head = raw[:len("|".join(HEADER)) + 1 + args.sample * (sum(WIDTHS) + len(WIDTHS))]
    t0 = time.perf_counter()
    np.loadtxt(io.BytesIO(head), delimiter="|", skiprows=1, dtype=np.int64, usecols=[HEADER.index(c) for c in KEYS])
    say(f"{step}: np.loadtxt on {args.sample} lines {(time.perf_counter() - t0) * 1e3:9.3f} ms (host, once)")


if args.step == "seoul":
    visits("seoul", args.seoul_rows, 100, 730, True)
elif args.step == "c3":
    visits("c3", args.rows, 100_000, 730, False)
else:
    T = args.float_rows
    g = torch.Generator(device=dev).manual_seed(2)
    for digits in (15, 19):
        cols = [torch.randint(10 ** (digits - 1), 10 ** digits - 1, (T if digits == 15 else T // 100,), device=dev, generator=g) for _ in range(3)]
        head = torch.tensor(list(b"x|y|z\n"), dtype=torch.uint8, device=dev)
        data = torch.cat([head, fixed_width(cols, (digits,) * 3)])
        name = f"floats, {digits} digits"
        say(f"{name}: {int(cols[0].numel())} lines, {int(data.numel())} bytes")
        t = timed(lambda: text.read_table(data, {"z": torch.float64, "x": torch.float64, "y": torch.float64}))
        say(f"{name}: read_table              {t * 1e3:9.3f} ms  {int(data.numel()) / t / 1e9:8.2f} GB/s")
