"""The Adam step (csrc/adam.hip, optim.Adam) beside torch's: how far ONE step lies from torch.optim.Adam's, and what a step costs.

  python tools/adam_lab.py --build     on the build machine, before the run: compiles csrc/adam.hip ALONE into tools/adam_lab_v<k>.so,
                                       k = 1..5, each with ONE operation of the per-element update contracted into a fused multiply-add
                                       (-DNGCF_ADAM_VARIANT=k: 1 g + wd * p, 2 m + c1 * (g - m), 3 fma(v, beta2, (c2 * g) * g),
                                       4 fma(c2 * g, g, v * beta2), 5 p + step_size * q).  A few seconds each; no GPU.
  python tools/adam_lab.py             the run.  Steps, each a child process of its own under `timeout` (a step that fails or runs
                                       out of time ends the run; the lines so far are kept):
    distance  `adam_oracle.distance_to_torch` (tests/adam_oracle.py: the function tests/test_adam_gpu.py holds the result of) against
              torch's default Adam and its capturable=True Adam, for the library's recipe and for every variant that was built
    c1        ms per optimizer step on the parameter set of bench.py's c1_train model (5 840 users x 100 items, embed 65, three layers
              of 65), gradients fixed: optim.Adam against torch's default, fused=True and capturable=True Adam, issued eagerly and as a
              captured graph of one step
    c1_graph  ms per training step of `GraphedTrainStep` on that model with optim.Adam and with torch's capturable Adam
    c3        ms per optimizer step on the C3 training parameter set (1.1 M x 130 embeddings plus the layers' weights)
Timings: device time between two events around --reps steps after --warmup, best of 3 such runs.
Writes its lines to --out (default profiles/adam_lab.txt) as well as to stdout."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = {"distance": 300, "c1": 300, "c1_graph": 300, "c3": 420}          # seconds allowed per step
VARIANTS = {1: "g + wd * p contracted", 2: "m + c1 * (g - m) contracted", 3: "fma(v, beta2, (c2 * g) * g)", 4: "fma(c2 * g, g, v * beta2)",
            5: "p + step_size * q contracted"}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_lab.txt"))
ap.add_argument("--build", action="store_true", help="compile the variant libraries and exit")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--only", choices=sorted(STEPS))
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the driver starts)")
args = ap.parse_args()

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def variant_lib(k):
    return os.path.join(HERE, f"adam_lab_v{k}.so")


if args.build:
    from seoul_tourism_recommendation_ngcf_amd import _build
    for k in VARIANTS:
        cmd = [_build._hipcc()] + _build.FLAGS + [f"-DNGCF_ADAM_VARIANT={k}", "-o", variant_lib(k), os.path.join(_build.CSRC, "adam.hip")]
        print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    sys.exit(0)

if args.step is None:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for step, limit in STEPS.items():
        if args.only and step != args.only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--out", args.out,
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            with open(args.out, "a") as f:
                f.write(f"step {step}: ended with exit status {rc}; nothing after it was run\n")
            sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402

import adam_oracle as orc  # noqa: E402
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402

eng = pkg.engine
dev = torch.device("cuda:0")


def say(s):
    print(s, flush=True)
    with open(args.out, "a") as f:
        f.write(s + "\n")


def device_ms(fn):
    """ms per call: events around --reps calls after --warmup, best of 3"""
    for _ in range(args.warmup):
        fn()
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.reps
        best = ms if best is None else min(best, ms)
    return best


def variant_step(path):
    """`engine.optim.adam_step`'s signature on a library that holds csrc/adam.hip alone."""
    lib = C.CDLL(path)
    fn = lib.ngcf_adam_step_f32
    fn.restype, fn.argtypes = pkg._lib.PROTOTYPES["ngcf_adam_step_f32"]

    def step(params, grads, exp_avgs, exp_avg_sqs, steps, ticket, *, lr, betas, eps, weight_decay, maximize):
        n = len(params)
        ptrs = [(C.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (params, grads, exp_avgs, exp_avg_sqs, steps)]
        numel = (C.c_int64 * n)(*[t.numel() for t in params])
        rc = fn(n, *ptrs, numel, eng._ptr(ticket), lr, betas[0], betas[1], eps, weight_decay, int(maximize), eng._stream())
        assert rc == 0, rc
    return step


def optimizers(params):
    return (("optim.Adam", lambda: pkg.optim.Adam(params, lr=1e-3)),
            ("torch Adam, default (foreach)", lambda: torch.optim.Adam(params, lr=1e-3)),
            ("torch Adam, fused=True", lambda: torch.optim.Adam(params, lr=1e-3, fused=True)),
            ("torch Adam, capturable=True", lambda: torch.optim.Adam(params, lr=1e-3, capturable=True)))


def time_parameter_set(name, shapes, graphs):
    g = torch.Generator(device=dev).manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
    n = sum(p.numel() for p in params)
    say(f"{name}: {len(params)} tensors, {n} elements ({n * 28 / 1e6:.1f} MB for one pass over p, g, m, v: 28 bytes per element)")
    for label, make in optimizers(params):
        opt = make()
        ms = device_ms(opt.step)
        line = f"  {label:32s} eager {ms:8.3f} ms per step"
        if graphs and all(grp.get("capturable") for grp in opt.param_groups):
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                opt.step()
            line += f", one captured step replayed {device_ms(graph.replay):8.3f} ms"
        say(line)
        del opt
        torch.cuda.empty_cache()


C1_SHAPES = [(5840, 65), (100, 65), (76, 13), (2, 13), (13, 13), (32, 13), (7, 13)] + [(65, 65), (65,), (65, 65), (65,)] * 3
C3_SHAPES = [(1_000_000, 130), (100_000, 130), (130, 128), (128,), (130, 128), (128,)] + [(128, 128), (128,), (128, 128), (128,)] * 2

if args.step == "distance":
    say(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    say(f"one-step distance to torch.optim.Adam, max over {orc.HELD_STEPS} steps on {list(orc.HELD_SHAPES)} in ulps of torch's result "
        f"(adam_oracle.distance_to_torch):")
    cases = [("recipe", eng.optim.adam_step)]
    cases += [(f"variant {k}: {what}", variant_step(variant_lib(k))) for k, what in VARIANTS.items() if os.path.exists(variant_lib(k))]
    for label, fn in cases:
        for capturable in (False, True):
            w = orc.distance_to_torch(fn, eng.optim.new_ticket, dev, capturable)
            say(f"  distance to torch capturable={capturable!s:5s} {label:45s} m {w['m']:6d}  v {w['v']:6d}  p {w['p']:6d}")
    if len(cases) == 1:
        say("  (no variant library was built: python tools/adam_lab.py --build)")
elif args.step == "c1":
    time_parameter_set("c1_train parameter set", C1_SHAPES, graphs=True)
elif args.step == "c3":
    time_parameter_set("C3 training parameter set", C3_SHAPES, graphs=False)
else:
    U, I, B = 5840, 100, 1024
    lap = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(dev, seed=1801, n_user=U, n_item=I)]
    num = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    gen = torch.Generator().manual_seed(3)
    r = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(dev)  # noqa: E731
    batch = dict(year=torch.full((B,), 18, device=dev), u_id=r(U), age=r(76), sex=r(2), month=r(13), day=r(32), dow=r(7), pos_item=r(I),
                 neg_item=r(I))
    say(f"GraphedTrainStep on the c1_train model ({U} users x {I} items, embed 65 -> [65, 65, 65], batch {B}), ms per replayed step:")
    for label, make in (("optim.Adam", lambda ps: pkg.optim.Adam(ps, lr=1e-3)),
                        ("torch Adam, capturable=True", lambda ps: torch.optim.Adam(ps, lr=1e-3, capturable=True))):
        torch.manual_seed(4)
        model = pkg.NGCF(65, [65, 65, 65], 0.3, [0.1, 0.1, 0.1], 1.0, lap, num, B, dev).to(dev).train()
        model.node_dropout_mode = model.mess_dropout_mode = "device"
        step = pkg.GraphedTrainStep(model, pkg.BPR(0.025, B), make(model.parameters()), batch)
        say(f"  {label:32s} {device_ms(lambda: step(**batch)):8.3f} ms per step, loss {float(step.loss):.6f}")
