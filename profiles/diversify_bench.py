"""Time MMR re-ranking and intra-list diversity on the device lists of dcue_topk (dcue_list_mmr /
dcue_list_ild through rank.Diversify) against the route a user would write in torch today, at BASELINE
config 2's serving shape, and print one JSON line.

  python3 profiles/diversify_bench.py [--reps 7] [--out profiles/diversify_bench.json]

Shape: 4,096 Gaussian users x 200,000 Gaussian tracks, d = 128, cosine scores; pool 128 -> k 100,
lambda = 0.7, raw relevance; ILD at K = 10, 50, 100 on the re-ranked lists.
  topk        TopK.topk_raw at k = 128 alone (the call synchronises its stream)
  topk+mmr    the same call followed by Diversify.mmr_raw
  mmr         Diversify.mmr_raw alone on the lists of a finished top-K call (ONE k_list_mmr launch)
  ild         Diversify.ild_raw + ild_mean_raw on the re-ranked lists (k_list_ild, k_list_ild_mean)
  torch mmr   on the same device lists: gather of the pool's rows [n, 128, d], F.normalize, bmm Gram
              [n, 128, 128], then the k-step loop of masked argmax and max updates -- fp32
  torch ild   gather + normalize + bmm of the re-ranked lists, the pair sums from the Gram's blocks
Device events around each call, every route warmed up, the routes alternating in one process; median
and min-max of each. Needs an MI355X: without a GPU it fails.

Agreement (asserted): at least 99 % of the fused lists' entries equal the torch loop's (both are fp32
routes with different summation orders; where two f values lie within rounding of each other a pick may
differ, and the rest of that list with it -- the bound is the 1 % step cap of tests/test_gpu_mmr.py),
and the mean ILD of the two routes agrees within (2 d + 16) 2^-24.

Not measured here: kernel time by rocprofv3 (a run of its own), other pool sizes, d and lambda, dot
scores with min-max relevance, and occupancy counters.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=200000)
    ap.add_argument("--n-users", type=int, default=4096)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--ild-ks", default="10,50,100")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    ks = [int(x) for x in args.ild_ks.split(",")]

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("diversify_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    n, n_cand, d, P, k, lam = args.n_users, args.n_cand, args.d, args.pool, args.k, args.lam

    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    cf = torch.randn(n_cand, d, generator=gen).to(dev)
    qf = torch.randn(n, d, generator=gen).to(dev)
    queries = np.arange(n)
    tk = rank.TopK(None, None, None, dev, n_cand=n_cand)
    div = rank.Diversify(dev)
    ar = torch.arange(n, device=dev)

    def topk():
        return tk.topk_raw(qf, cf, queries, P)

    pool = topk()

    def mmr():
        return div.mmr_raw(pool[0], pool[1], pool[2], cf, k, lam, "raw")

    def topk_mmr():
        idx, score, count, _ = topk()
        return div.mmr_raw(idx, score, count, cf, k, lam, "raw")

    picked = mmr()

    def ild():
        v, flags = div.ild_raw(picked[0], picked[2], cf, ks)
        return div.ild_mean_raw(v, flags)

    def gram(idx):
        rows = F.normalize(cf[idx.long()], dim=2, eps=1e-8)  # [n, len, d]
        return torch.bmm(rows, rows.transpose(1, 2))

    def torch_mmr():
        idx, rel = pool[0], pool[1]
        S = gram(idx)
        taken = torch.zeros((n, P), dtype=torch.bool, device=dev)
        m = torch.zeros((n, P), device=dev)
        out = torch.empty((n, k), dtype=torch.int64, device=dev)
        for t in range(k):
            f = (lam * rel - (1.0 - lam) * m).masked_fill(taken, float("-inf"))
            a = f.argmax(dim=1)
            out[:, t] = a
            taken[ar, a] = True
            row = S[ar, a]
            m = row if t == 0 else torch.maximum(m, row)
        return idx.gather(1, out.to(torch.int64)).to(torch.int32), rel.gather(1, out)

    def torch_ild():
        S = gram(picked[0])
        vals = []
        for K in ks:
            blk = S[:, :K, :K]
            pairs = ((1.0 - blk).sum((1, 2)) - (1.0 - torch.diagonal(blk, dim1=1, dim2=2)).sum(1)) / 2
            vals.append(pairs * (2.0 / (K * (K - 1))))
        return torch.stack(vals, 1).mean(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    routes = {"topk": topk, "topk_mmr": topk_mmr, "mmr": mmr, "ild": ild, "torch_mmr": torch_mmr,
              "torch_ild": torch_ild}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn))
    peak = torch.cuda.max_memory_allocated() - base_mem

    # agreement (module docstring)
    t_idx, _ = torch_mmr()
    same = float((t_idx == picked[0]).float().mean())
    ild_f = ild()[0].cpu().numpy()
    ild_t = torch_ild().double().cpu().numpy()
    ild_pool = div.ild_mean_raw(*div.ild_raw(pool[0], pool[2], cf, ks))[0].cpu().numpy()
    tol = (2 * ((d + 15) // 16 * 16) + 16) * 2.0 ** -24
    agreement = {"entries_equal_to_torch": same, "ild_fused": ild_f.tolist(), "ild_torch": ild_t.tolist(),
                 "ild_max_abs_diff": float(np.abs(ild_f - ild_t).max()), "ild_tolerance": tol,
                 "ild_of_the_plain_ranking": ild_pool.tolist()}
    print("agreement: %s" % json.dumps(agreement), file=sys.stderr)
    assert not bool(picked[3].any()) and bool((picked[2] == k).all())
    assert same >= 0.99, same
    assert np.abs(ild_f - ild_t).max() <= tol, (ild_f, ild_t)

    def stat(name):
        t = times[name]
        return {"median": float(np.median(t)), "min": min(t), "max": max(t)}

    def spread(name):
        return max(times[name]) - min(times[name])

    med = {name: float(np.median(t)) for name, t in times.items()}
    res = {
        "bench": "diversify", "device": torch.cuda.get_device_name(0),
        "shape": {"n_users": n, "n_cand": n_cand, "d": d, "pool": P, "k": k, "lambda": lam, "rel": "raw",
                  "score": "cosine", "ild_ks": ks},
        "reps": args.reps, "warmup": args.warmup,
        "ms": {name: stat(name) for name in routes},
        "mmr_share_of_topk": med["mmr"] / med["topk"],
        "topk_mmr_over_topk": med["topk_mmr"] / med["topk"],
        "torch_mmr_over_fused": med["torch_mmr"] / med["mmr"],
        "torch_ild_over_fused": med["torch_ild"] / med["ild"],
        "mmr_faster_beyond_noise": bool(med["torch_mmr"] - med["mmr"] > max(spread("mmr"), spread("torch_mmr"))),
        "ild_faster_beyond_noise": bool(med["torch_ild"] - med["ild"] > max(spread("ild"), spread("torch_ild"))),
        "mmr_us_per_list": med["mmr"] * 1e3 / n,
        "mmr_row_read_gbps": n * P * d * 4 / (med["mmr"] * 1e-3) / 1e9,
        "torch_launches_per_mmr_call": "about 7 per step x k steps + gather, normalize, bmm",
        "torch_peak_bytes": int(peak),
        "fused_workspace_bytes": 0,
        "agreement": agreement,
        "not_measured": ["kernel time by rocprofv3", "other pool sizes, d and lambda", "dot scores with min-max "
                         "relevance", "occupancy counters"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
