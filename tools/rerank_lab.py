"""Diversifying re-rank lab: engine.lists.mmr_rerank against the same greedy MMR from torch ops.

    python tools/rerank_lab.py [--out profiles/rerank_lab.txt] [--skip-c3] [--c3-users N] [--reps R]

Two shapes.  C3: tables of C3's size - 1 M pools x n = 64 over 100 K items, item embeddings [100 K, 512] N(0, 1), top = 20 - with the
ids drawn from a skewed popularity (u^3 over the catalogue) and descending N(0, 1) relevances; no model is propagated.  Seoul: the
Seoul-shaped stand-in's own pools (graphs.seoul_standin, 5 840 users x 100 items, D = 193; rank_topk with the training items
excluded, n = 64, top = 20).

The torch side is the formulation the kernel replaces: per chunk of pools a [chunk, n, D] gather, a bmm, the cosines, and a loop of
`top` steps over masked [chunk, n] tensors (argmax, gather of the picked column, running maximum).  Both sides run in one process,
alternating, `--reps` timed rounds after 2 warm-up rounds, device events, medians.  Peak memory is torch's allocator peak over one
call of each side; the kernel's gathered bytes per second count n * D * 4 bytes per pool.  evaluate.list_quality's ild@20 and
novelty are reported for the pools' first 20 columns and for the re-ranked lists at lam = 0.7.
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
LAM = 0.7


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


def torch_mmr(pool, rel, items, top, lam, chunk):
    """Greedy MMR in torch ops, min-max normalised relevance, fp32 Gram like the kernel's, cosines and keys in fp64."""
    out = torch.empty((pool.shape[0], top), dtype=torch.int64, device=pool.device)
    for c0 in range(0, pool.shape[0], chunk):
        ids = pool[c0:c0 + chunk]
        ok = ids >= 0
        E = items[ids.clamp(min=0)] * ok[..., None]
        G = torch.bmm(E, E.transpose(1, 2)).double()
        d = torch.diagonal(G, dim1=1, dim2=2)
        p = d[:, :, None] * d[:, None, :]
        cos = torch.where(p == 0, torch.zeros_like(G), G / p.sqrt())
        v = rel[c0:c0 + chunk].double()
        fin = ok & torch.isfinite(v)
        lo = torch.where(fin, v, torch.full_like(v, float("inf"))).min(1, keepdim=True).values
        hi = torch.where(fin, v, torch.full_like(v, float("-inf"))).max(1, keepdim=True).values
        r = torch.where(hi > lo, (v - lo) / (hi - lo), torch.zeros_like(v))
        cand = ok.clone()
        m = torch.zeros_like(v)
        rows = torch.arange(ids.shape[0], device=pool.device)
        for t in range(top):
            key = lam * r if t == 0 else lam * r - (1.0 - lam) * m
            key = torch.where(cand, key, torch.full_like(key, float("-inf")))
            s = key.argmax(1)
            any_left = cand.any(1)
            out[c0:c0 + chunk, t] = torch.where(any_left, ids[rows, s], torch.full_like(s, -1))
            cand[rows, s] = False
            c = cos[rows, :, s]
            m = c if t == 0 else torch.maximum(m, c)
    return out


def compare(name, pool, rel, items, top, reps, chunk):
    dev = pool.device
    B, n = int(pool.shape[0]), int(pool.shape[1])
    n_items, D = int(items.shape[0]), int(items.shape[1])
    say(f"{name}: {B} pools x n = {n}, top = {top}, lam = {LAM}, {n_items} items, D = {D}, row pitch {items.stride(0)} floats")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {}
    t_o, t_t, r_o, r_t, peaks = alternating(
        lambda: res.__setitem__("o", eng.lists.mmr_rerank(pool, rel, items, top, lam=LAM, status=status)),
        lambda: res.__setitem__("t", torch_mmr(pool, rel, items, top, LAM, chunk)), reps)
    same = float((res["o"] == res["t"]).all(1).double().mean())
    gathered = float((pool >= 0).sum()) * D * 4
    say(f"  mmr_rerank        {t_o:9.3f} ms [{r_o[0]:.3f}, {r_o[1]:.3f}] peak {peaks[0]:8.1f} MiB | torch gather + bmm + {top} masked argmax "
        f"steps, chunks of {chunk} {t_t:9.3f} ms [{r_t[0]:.3f}, {r_t[1]:.3f}] peak {peaks[1]:8.1f} MiB")
    say(f"    gathered {gathered / 1e9:.2f} GB of item rows -> {gathered / (t_o * 1e-3) / 1e9:.0f} GB/s; lists equal to the torch side's: "
        f"{same * 100:.3f} % (torch's bmm sums in another order: near-ties may fall the other way)")
    assert int(status) == 0
    return res["o"]


def quality(name, before, after, items, pop, n_user):
    """ild@20 and novelty of two sets of lists through engine.lists (what evaluate.list_quality computes for lists=)."""
    n_items = int(items.shape[0])
    for label, top in (("pool's first 20", before), (f"re-ranked, lam = {LAM}", after)):
        ild = eng.lists.list_diversity(top, items, (20,))["ild@20"]
        fig = eng.lists.exposure_summary(eng.lists.exposure_counts(top, n_items), pop, n_user)
        say(f"  {name} {label:24s} ild@20 {ild:.6f}  novelty {fig['novelty']:.6f} bits  coverage {fig['coverage']:.6f}")


def c3(dev, n_pools, reps):
    n_items, D, n, top = 100_000, 512, 64, 20
    g = torch.Generator(device=dev).manual_seed(2604)
    items = torch.randn((n_items, D), generator=g, device=dev)
    pool = (torch.rand((n_pools, n), generator=g, device=dev) ** 3 * n_items).long().clamp(max=n_items - 1)
    rel = torch.sort(torch.randn((n_pools, n), generator=g, device=dev), 1, descending=True).values
    pop = (torch.rand(n_items, generator=g, device=dev) * 2000).long()
    out = compare("C3 sizes", pool, rel, items, top, reps, 8192)
    quality("C3 sizes", pool[:, :20].contiguous(), out, items, pop, 1_000_000)


def seoul(dev, reps):
    n_user, n_item = 5840, 100
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(dev)]
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    model = pkg.NGCF(65, [64, 64], None, None, 1.0, laps, num_dict, 256, dev).to(dev).eval()
    train = eng.ItemSets.from_laplacian(model.laplacian_csr(0), n_user)
    with torch.no_grad():
        model.propagate(0)
        vals, pool = eng.rank_topk(model.all_users_emb, model.all_items_emb, 64, exclude=train)
    pop = eng.lists.exposure_counts((train.colidx.to(torch.int64) - train.col_offset).reshape(-1, 1), n_item)
    out = compare("Seoul stand-in", pool, vals, model.all_items_emb, 20, reps, 8192)
    quality("Seoul stand-in", pool[:, :20].contiguous(), out, model.all_items_emb, pop, n_user)
    users = torch.arange(n_user, device=dev)
    res = {}
    once(lambda: res.__setitem__("q", pkg.recommend.diversified_ranking(model, users, train=train, lam=LAM, pool=64, top=20)))
    t = once(lambda: res.__setitem__("q", pkg.recommend.diversified_ranking(model, users, train=train, lam=LAM, pool=64, top=20)))
    say(f"  recommend.diversified_ranking(pool=64, top=20), propagate and ranking included: {t:.2f} ms; equal to the two calls: "
        f"{bool(torch.equal(res['q'][0], out))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rerank_lab.txt")
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--c3-users", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    say(f"rerank_lab on {torch.cuda.get_device_name(0)}; medians of {args.reps} alternating rounds after 2 warm-up rounds, [min, max]")
    seoul(dev, args.reps)
    if not args.skip_c3:
        c3(dev, args.c3_users, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
