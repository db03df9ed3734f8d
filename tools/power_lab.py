"""The Yeo-Johnson power scaler's fit on the device (preprocess.fit_power: Brent on the host, one engine.yeo_johnson_moments launch
per evaluation of the likelihood) against the same likelihood from torch ops and against sklearn's PowerTransformer.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  c3       --rows = 50 M rows of heavy-tailed integer counts (floor(exp(N(3, 1.5)))): fit_power timed whole, the evaluations it took,
           ms per evaluation (the moments kernel alone, device events), the elementwise transform, and the same likelihood value
           from torch ops (where / pow / log1p / var: about six passes over the column with temporaries).
  seoul    the Seoul-shaped stand-in's rows (graphs.seoul_standin) with such counts: the same.
  sklearn  PowerTransformer().fit on the Seoul shape, host only; skipped with a line that says so where sklearn is missing.
The lambda of the torch-ops likelihood minimised by the same host loop is compared with fit_power's before anything is timed.
Writes its lines to --out (default profiles/power_lab.txt) as well as to stdout."""
import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"c3": 600, "seoul": 180, "sklearn": 300}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_lab.txt"))
ap.add_argument("--rows", type=int, default=50_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the driver starts)")
args = ap.parse_args()

if args.step is None:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for step, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out,
               "--rows", str(args.rows), "--reps", str(args.reps)]
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


def counts_like(n, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.floor(torch.exp(torch.randn(n, generator=g, device=device, dtype=torch.float64) * 1.5 + 3.0))


def torch_likelihood(x, c, lam):
    """f(lam) from torch ops, the header's statement of psi: x is float64 without NaNs, c its lambda-free term."""
    pos = x >= 0
    if abs(lam) < 2.0 ** -52:
        yp = torch.log1p(x)
    else:
        yp = (torch.pow(x + 1, lam) - 1) / lam
    if abs(lam - 2) <= 2.0 ** -52:
        yn = -torch.log1p(-x)
    else:
        yn = -(torch.pow(-x + 1, 2 - lam) - 1) / (2 - lam)
    var = float(torch.where(pos, yp, yn).var(unbiased=False))
    n = x.numel()
    return math.inf if var < 2.2250738585072014e-308 else n / 2 * math.log(var) - (lam - 1) * c


def device_side(name, counts):
    T = int(counts.numel())
    say(f"{name}: {T} rows, max count {int(counts.max())}")
    x = counts.to(torch.float64).contiguous()
    evals = [0]
    real = eng.yeo_johnson_moments

    def counting(xx, lam):
        evals[0] += 1
        return real(xx, lam)
    eng.yeo_johnson_moments = counting
    t0 = time.perf_counter()
    ps = pre.fit_power(x)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    eng.yeo_johnson_moments = real
    say(f"  fit_power (first call): lambda {ps.lam:.9f}, {evals[0]} evaluations, {wall:.1f} ms wall = {wall / evals[0]:.2f} ms per evaluation "
        "with its read-back; the standardisation of psi is in the total")
    c = float(torch.sum(torch.sign(x) * torch.log1p(torch.abs(x))))
    lam_t = pre._brent(lambda lam: torch_likelihood(x, c, lam), (-2.0, 2.0), 1.48e-8, 500)
    say(f"  lambda from the torch-ops likelihood through the same host loop: {lam_t:.9f} (difference {ps.lam - lam_t:+.2e})")
    ms = timed(lambda: pre.fit_power(x), max(2, args.reps // 2))
    say(f"  fit_power: {fmt(ms)}")
    ms_k = timed(lambda: real(x, ps.lam), args.reps)
    blocks, threads, _ = eng.yeo_johnson_launch(T)
    say(f"  one evaluation, engine.yeo_johnson_moments ({blocks} x {threads} threads + 1 workgroup): {fmt(ms_k)} = "
        f"{8 * T / np.median(ms_k) / 1e6:.1f} GB/s of column read, {T / np.median(ms_k) / 1e6:.2f} G pow/s")
    ms = timed(lambda: eng.yeo_johnson(x, ps.lam), args.reps)
    say(f"  the transform, engine.yeo_johnson: {fmt(ms)} = {16 * T / np.median(ms) / 1e6:.1f} GB/s read + written")
    ms = timed(lambda: torch_likelihood(x, c, ps.lam), max(2, args.reps // 2))
    say(f"  the same likelihood from torch ops: {fmt(ms)} = {np.median(ms) / np.median(ms_k):.1f}x one fused evaluation")


def seoul_counts(device):
    coo = pkg.graphs.seoul_standin(device)[0]
    n = int((coo["rows"] < coo["n_user"]).sum())
    return counts_like(n, device, 5)


if args.step == "c3":
    device_side("C3 shape", counts_like(args.rows, torch.device("cuda:0"), 2603))
elif args.step == "seoul":
    device_side("Seoul-shaped stand-in", seoul_counts(torch.device("cuda:0")))
else:
    try:
        from sklearn.preprocessing import PowerTransformer
    except ImportError:
        say("sklearn is not installed: PowerTransformer was not timed")
        sys.exit(0)
    x = seoul_counts("cpu").numpy().reshape(-1, 1)
    t0 = time.perf_counter()
    pt = PowerTransformer().fit(x)
    say(f"sklearn PowerTransformer().fit, Seoul shape ({len(x)} rows), host: {(time.perf_counter() - t0) * 1e3:.1f} ms, lambda {pt.lambdas_[0]:.9f}")
