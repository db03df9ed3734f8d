"""The two builders of the year-slice Laplacians side by side: `matrix.laplacian_slices` (torch ops, int64 COO out - unchanged, so
its time is the yardstick) and `matrix.laplacian_csr_slices` (csrc/laplacian.hip, int32 CSR out).

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the run; the lines so far are kept):
  seoul   Seoul-shaped stand-in (graphs.seoul_standin: 5 840 users x 100 items, two years, the second overlaying the first).
  c3      C3 shape (1 M users x 100 K items, --inter = 50 M draws, de-duplicated) split into two years, records shuffled with a
          year-18 record first: the input of tests/test_matrix.py::test_matrix_builder_at_c3_scale_on_device.
Per shape and builder: wall time of one build of both slices from records already on the device (what `Matrix.create_matrix` does
after the frame's columns are uploaded), host clock around a synchronised call, median of --reps after one warm-up;
`torch.cuda.max_memory_allocated` over one build, above what the records themselves hold; and the time to the engine's CSR of the
last slice (`LaplacianCSR.from_coo` of the COO, as `NGCF.laplacian_csr` does, against `LaplacianSlice.csr()`).  The two results
are compared entry for entry before anything is timed.
Writes its lines to --out (default profiles/laplacian_lab.txt) as well as to stdout."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"seoul": 240, "c3": 900}          # seconds allowed per step

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplacian_lab.txt"))
ap.add_argument("--inter", type=int, default=50_000_000)
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
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out,
               "--inter", str(args.inter), "--reps", str(args.reps)]
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
from seoul_tourism_recommendation_ngcf_amd import matrix  # noqa: E402

eng = pkg.engine


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


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p / 2 ** 20


def compare(name, year, u, i, w, n_user, n_item):
    dev = year.device
    N = n_user + n_item
    say(f"{name}: {n_user} users x {n_item} items, {int(year.numel())} records in {int(torch.unique(year).numel())} years")
    torch_build = lambda: matrix.laplacian_slices(year, u, i, w, n_user, n_item, device=dev)  # noqa: E731
    hip_build = lambda: matrix.laplacian_csr_slices(year, u, i, w, n_user, n_item, dev)  # noqa: E731
    want, got = torch_build(), hip_build()
    same = sorted(want) == sorted(got)
    for k in want:
        rows, cols, vals = got[k].coo()
        same = same and torch.equal(rows, want[k][0]) and torch.equal(cols, want[k][1]) and torch.equal(vals.view(torch.int32),
                                                                                                        want[k][2].view(torch.int32))
        got[k]._rows = None
    last = max(want)
    say(f"  slices equal bit for bit: {same}; entries of the last slice: {int(want[last][0].numel())}")
    coo, sl = want[last], got[last]
    del want, got
    t_conv = wall(lambda: eng.LaplacianCSR.from_coo(*coo, N, N), args.reps)
    t_csr = wall(lambda: sl.csr(), args.reps)
    del coo, sl
    t_torch, t_hip = [], []
    for _ in range(args.reps):                                       # alternating, so that both see the same neighbours
        t_torch += wall(torch_build, 1, warm=0)
        t_hip += wall(hip_build, 1, warm=0)
    m_torch, m_hip = peak(torch_build), peak(hip_build)
    ratio = np.median(t_torch) / np.median(t_hip)
    spread = max(max(t_torch) / min(t_torch), max(t_hip) / min(t_hip)) - 1.0
    say(f"  laplacian_slices (torch ops, the yardstick):  {fmt(t_torch)}; peak {m_torch:.0f} MiB above the records")
    say(f"  laplacian_csr_slices (HIP):                   {fmt(t_hip)}; peak {m_hip:.0f} MiB above the records")
    say(f"  torch / HIP = {ratio:.2f}x; run-to-run spread (max / min - 1, the larger of the two) {spread * 100:.0f} %: "
        + ("the HIP builder is faster by more than the spread" if ratio > 1.0 + spread else
           "the HIP builder is NOT faster by more than the spread"))
    say(f"  to the engine's CSR, last slice: LaplacianCSR.from_coo {fmt(t_conv)}; LaplacianSlice.csr() {fmt(t_csr)}")


dev = torch.device("cuda:0")
if args.step == "seoul":
    ys, us, its, ws = [], [], [], []
    for k, coo in enumerate(pkg.graphs.seoul_standin(dev)):          # a year's records: the user rows of its slice (values are not ratings,
        sel = coo["rows"] < coo["n_user"]                            # but non-zero weights of the same pattern)
        us.append(coo["rows"][sel].to(torch.int64))
        its.append((coo["cols"][sel] - coo["n_user"]).to(torch.int64))
        ws.append(coo["vals"][sel].to(torch.float32))
        ys.append(torch.full((int(sel.sum()),), 18 + k, dtype=torch.int64, device=dev))
    n_user, n_item = int(coo["n_user"]), int(coo["n_item"])
    year, u, i, w = (torch.cat(a) for a in (ys, us, its, ws))
else:
    n_user, n_item = 1_000_000, 100_000
    u, i, w = pkg.graphs.synthetic_interactions(n_user, n_item, args.inter, seed=2603, device=dev)
    n = int(u.numel())
    year = torch.cat([torch.full((n // 2,), 18, device=dev), torch.full((n - n // 2,), 19, device=dev)])
perm = torch.randperm(int(year.numel()), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
k = int((year[perm] == 18).nonzero()[0])
perm[[0, k]] = perm[[k, 0]]
year, u, i, w = year[perm].contiguous(), u[perm].contiguous(), i[perm].contiguous(), w[perm].contiguous()
del perm
compare("Seoul-shaped stand-in" if args.step == "seoul" else "C3 shape", year, u, i, w, n_user, n_item)
