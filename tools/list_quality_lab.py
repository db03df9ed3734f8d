"""Beyond-accuracy list figures lab: engine.lists' three calls against the same figures from torch ops.

    python tools/list_quality_lab.py [--out profiles/list_quality_lab.txt] [--skip-c3] [--c3-users N] [--reps R]

Two shapes.  C3: tables of C3's size - 1 M lists x k = 20 over 100 K items, item embeddings [100 K, 512] N(0, 1) - with the ids drawn
from a skewed popularity (u^3 over the catalogue), so that the exposure histogram has a head and a tail; the figures depend on the
ids and the table alone, no model is propagated.  Seoul: the Seoul-shaped stand-in's own lists (graphs.seoul_standin, 5 840 users x
100 items, embed 65 -> [64, 64], D = 193; rank_topk with the training items excluded, k = 20).

Per shape each of the three calls - exposure_counts, exposure_summary, list_diversity - is timed against its torch formulation
(bincount; sort, cumsum and log2 on the histogram; a chunked [chunk, k, D] gather, normalise and bmm) in one process, the two sides
alternating, `--reps` timed rounds after 2 warm-up rounds, device events, medians.  Peak memory is torch's allocator peak over one
call of each side; the diversity kernel's gathered bytes per second count k * D * 4 bytes per list.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seoul_tourism_recommendation_ngcf_amd as pkg  # noqa: E402
from seoul_tourism_recommendation_ngcf_amd import engine as eng  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)                 # ms


def alternating(ours, theirs, reps):
    """Median ms of each side over `reps` rounds, ours and theirs taking turns, after 2 warm-up rounds; and each side's allocator
    peak above what was allocated before its call."""
    peaks = []
    for fn in (ours, theirs):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks.append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
    ours()
    theirs()
    t_ours, t_theirs = [], []
    for _ in range(reps):
        t_ours.append(once(ours))
        t_theirs.append(once(theirs))
    return statistics.median(t_ours), statistics.median(t_theirs), (min(t_ours), max(t_ours)), (min(t_theirs), max(t_theirs)), peaks


def torch_counts(top, n_items):
    flat = top.reshape(-1)
    return torch.bincount(flat[flat >= 0], minlength=n_items)


def torch_summary(counts, pop, n_user):
    n = counts.numel()
    c = torch.sort(counts).values
    total = c.sum()
    weighted = (c * torch.arange(1, n + 1, device=c.device)).sum()
    cd = counts.double()
    clog = torch.where(counts > 0, cd * torch.log2(cd.clamp(min=1.0)), torch.zeros_like(cd)).sum()
    nov = (cd * (torch.log2(torch.tensor(float(n_user), dtype=torch.float64, device=c.device)) - torch.log2(pop.clamp(min=1).double()))).sum()
    return torch.stack(((counts > 0).sum().double(), total.double(), weighted.double(), clog, nov)).cpu()


def torch_diversity(top, items, K, chunk):
    """Mean over the lists of the mean 1 - cos over the pairs of non-empty slots below K: a [chunk, K, D] gather, row norms and a
    bmm per chunk, fp32 Gram like the kernel's, cosines in fp64."""
    total = torch.zeros((), dtype=torch.float64, device=top.device)
    lists = torch.zeros((), dtype=torch.float64, device=top.device)
    upper = torch.triu(torch.ones((K, K), dtype=torch.bool, device=top.device), 1)
    for c0 in range(0, top.shape[0], chunk):
        ids = top[c0:c0 + chunk, :K]
        ok = ids >= 0
        E = items[ids.clamp(min=0)] * ok[..., None]
        G = torch.bmm(E, E.transpose(1, 2)).double()
        d = torch.diagonal(G, dim1=1, dim2=2)
        p = d[:, :, None] * d[:, None, :]
        cos = torch.where(p == 0, torch.zeros_like(G), G / p.sqrt())
        pair = ok[:, :, None] & ok[:, None, :] & upper
        V = ok.sum(1).double()
        n_pairs = V * (V - 1) / 2
        s = torch.where(pair, 1.0 - cos, torch.zeros_like(cos)).sum((1, 2))
        counted = n_pairs > 0
        total += torch.where(counted, s / n_pairs.clamp(min=1.0), torch.zeros_like(s)).sum()
        lists += counted.sum()
    return torch.stack((total, lists)).cpu()


def compare(name, top, items, pop, n_user, reps, chunk):
    dev = top.device
    B, k = int(top.shape[0]), int(top.shape[1])
    n_items, D = int(items.shape[0]), int(items.shape[1])
    tier = "LDS tables" if n_items <= eng.lists.EXPOSURE_LDS_ITEMS else "atomics in memory"
    say(f"{name}: {B} lists x k = {k}, {n_items} items ({tier}), D = {D}, row pitch {items.stride(0)} floats")
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    res = {}
    t_o, t_t, r_o, r_t, peaks = alternating(lambda: res.__setitem__("o", eng.lists.exposure_counts(top, n_items, status=status)),
                                            lambda: res.__setitem__("t", torch_counts(top, n_items)), reps)
    assert torch.equal(res["o"], res["t"])
    say(f"  exposure_counts   {t_o:9.3f} ms [{r_o[0]:.3f}, {r_o[1]:.3f}] peak {peaks[0]:8.1f} MiB | torch.bincount          {t_t:9.3f} ms "
        f"[{r_t[0]:.3f}, {r_t[1]:.3f}] peak {peaks[1]:8.1f} MiB | counts equal")
    counts = res["o"]

    t_o, t_t, r_o, r_t, peaks = alternating(lambda: res.__setitem__("o", eng.lists.exposure_summary(counts, pop, n_user)),
                                            lambda: res.__setitem__("t", torch_summary(counts, pop, n_user)), reps)
    o, t = res["o"], res["t"].tolist()
    say(f"  exposure_summary  {t_o:9.3f} ms [{r_o[0]:.3f}, {r_o[1]:.3f}] peak {peaks[0]:8.1f} MiB | torch sort/cumsum/log2 {t_t:9.3f} ms "
        f"[{r_t[0]:.3f}, {r_t[1]:.3f}] peak {peaks[1]:8.1f} MiB | both with their read-back")
    say(f"    coverage {o['coverage']:.6f} gini {o['gini']:.6f} entropy {o['entropy']:.6f} bits novelty {o['novelty']:.6f} bits; "
        f"clog relative difference {abs(o['clog'] - t[3]) / abs(t[3]):.1e}, nov {abs(o['nov'] - t[4]) / abs(t[4]):.1e}, integers equal: "
        f"{(o['covered'], o['total'], o['weighted']) == (int(t[0]), int(t[1]), int(t[2]))}")

    sums = torch.zeros(2, dtype=torch.float64, device=dev)

    def ours():
        sums.zero_()
        eng.lists.list_diversity(top, items, (k,), sums=sums, status=status)
    t_o, t_t, r_o, r_t, peaks = alternating(ours, lambda: res.__setitem__("t", torch_diversity(top, items, k, chunk)), reps)
    s, t = sums.cpu().tolist(), res["t"].tolist()
    gathered = float((top >= 0).sum()) * D * 4
    say(f"  list_diversity    {t_o:9.3f} ms [{r_o[0]:.3f}, {r_o[1]:.3f}] peak {peaks[0]:8.1f} MiB | torch gather + bmm, chunks of {chunk} "
        f"{t_t:9.3f} ms [{r_t[0]:.3f}, {r_t[1]:.3f}] peak {peaks[1]:8.1f} MiB")
    say(f"    ild@{k} {s[0] / max(s[1], 1):.9f} over {int(s[1])} lists (torch {t[0] / max(t[1], 1):.9f} over {int(t[1])}); gathered "
        f"{gathered / 1e9:.2f} GB of item rows -> {gathered / (t_o * 1e-3) / 1e9:.0f} GB/s; the torch side gathers the same rows in pieces "
        f"of {chunk * k * D * 4 / 2 ** 20:.0f} MiB")
    assert int(status) == 0


def c3(dev, n_lists, reps):
    n_items, D, k = 100_000, 512, 20
    g = torch.Generator(device=dev).manual_seed(2603)
    items = torch.randn((n_items, D), generator=g, device=dev)
    top = (torch.rand((n_lists, k), generator=g, device=dev) ** 3 * n_items).long().clamp(max=n_items - 1)
    pop = (torch.rand(n_items, generator=g, device=dev) * 2000).long()
    compare("C3 sizes", top, items, pop, 1_000_000, reps, 16384)


def seoul(dev, reps):
    n_user, n_item = 5840, 100
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(dev)]
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    model = pkg.NGCF(65, [64, 64], None, None, 1.0, laps, num_dict, 256, dev).to(dev).eval()
    train = eng.ItemSets.from_laplacian(model.laplacian_csr(0), n_user)
    with torch.no_grad():
        model.propagate(0)
        _, top = eng.rank_topk(model.all_users_emb, model.all_items_emb, 20, exclude=train)
    pop = eng.lists.exposure_counts((train.colidx.to(torch.int64) - train.col_offset).reshape(-1, 1), n_item)
    compare("Seoul stand-in", top, model.all_items_emb, pop, n_user, reps, 16384)
    res = {}
    t = once(lambda: res.__setitem__("q", pkg.evaluate.list_quality(model, train, ks=(5, 20))))
    t = once(lambda: res.__setitem__("q", pkg.evaluate.list_quality(model, train, ks=(5, 20))))
    say(f"  evaluate.list_quality(ks=(5, 20)), propagate and ranking included: {t:.2f} ms   {res['q'][20]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/list_quality_lab.txt")
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--c3-users", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say(f"list_quality_lab on {torch.cuda.get_device_name(0)}; medians of {args.reps} alternating rounds after 2 warm-up rounds, [min, max]")
    seoul(dev, args.reps)
    if not args.skip_c3:
        c3(dev, args.c3_users, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
