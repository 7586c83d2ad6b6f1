"""Time the explanation of served lists on the device lists of dcue_topk (dcue_list_explain through
rank.Explain) against the route a user would write in torch today, at BASELINE config 2's serving
shape, and print one JSON line.

  python3 profiles/explain_bench.py [--reps 7] [--out profiles/explain_bench.json]

Shape: 4,096 Gaussian users x 200,000 Gaussian tracks, d = 128, cosine scores, k = 100 picks per user,
histories of 20..80 songs (50 on average; the top-K call's exclusion rows), 3 reasons per pick.
  topk          TopK.topk_raw at k = 100 alone (the call synchronises its stream)
  explain       Explain.explain_raw alone on the lists of a finished top-K call: k_rank_normalize over the
                whole table into the workspace, then ONE k_list_explain launch
  topk+explain  the two calls back to back
  torch         on the same device lists: index_select of the lists' rows [n, k, d] and of the histories
                padded to the longest [n, Hmax, d], F.normalize, bmm [n, k, Hmax], padding to -inf, topk --
                fp32
  heavy tail    explain alone with 8 of the users given 5,000 plays each (one workgroup per list
                serialises a long history); torch is not run there (the padded gather would take 10 GB)
Device events around each call, every route warmed up, the routes alternating in one process; median
and min-max of each. Needs an MI355X: without a GPU it fails.

Agreement (asserted): at least 99 % of the fused reasons equal torch's (both are fp32 routes with different
summation orders; near-ties may swap), and the similarities agree position by position within
2 (rank_dp(d) + 8) 2^-24.

Not measured here: kernel time by rocprofv3 (a run of its own, so the split between the normalisation
pass and k_list_explain), other k, d, m and history lengths, masked histories, and occupancy counters.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))


def histories(rs, n, n_cand, lo, hi, heavy=0, heavy_len=0):
    """CSR of n sorted repeat-free rows of lo..hi draws (a repeated draw counts once); the first `heavy`
    rows take heavy_len draws instead."""
    lens = rs.randint(lo, hi + 1, n)
    lens[:heavy] = heavy_len
    rows = [np.unique(rs.randint(0, n_cand, int(ln))) for ln in lens]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.concatenate(rows).astype(np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=200000)
    ap.add_argument("--n-users", type=int, default=4096)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reasons", type=int, default=3)
    ap.add_argument("--plays", default="20,80")
    ap.add_argument("--heavy-users", type=int, default=8)
    ap.add_argument("--heavy-plays", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    lo, hi = [int(x) for x in args.plays.split(",")]

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    n, n_cand, d, k, m = args.n_users, args.n_cand, args.d, args.k, args.reasons

    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    cf = torch.randn(n_cand, d, generator=gen).to(dev)
    qf = torch.randn(n, d, generator=gen).to(dev)
    rs = np.random.RandomState(args.seed)
    queries = np.arange(n)
    q_dev = torch.from_numpy(queries.astype(np.int32)).to(dev)
    ptr, idx = histories(rs, n, n_cand, lo, hi)
    tk = rank.TopK(ptr, idx, None, dev, n_cand=n_cand)
    ex = rank.Explain(dev)
    hist = (tk.excl_ptr, tk.excl_idx)  # the CSR the top-K call already uploaded
    hptr, hidx = histories(rs, n, n_cand, lo, hi, args.heavy_users, args.heavy_plays)
    heavy = rank._upload_csr(hptr, hidx, dev)

    def topk():
        return tk.topk_raw(qf, cf, queries, k)

    lists = topk()

    def explain():
        return ex.explain_raw(lists[0], lists[2], q_dev, *hist, cf, m)

    def topk_explain():
        i, _, c, _ = topk()
        return ex.explain_raw(i, c, q_dev, *hist, cf, m)

    def explain_heavy():
        return ex.explain_raw(lists[0], lists[2], q_dev, *heavy, cf, m)

    lens = np.diff(ptr)
    hmax = int(lens.max())
    pad = np.full((n, hmax), -1, np.int64)
    for u in range(n):
        pad[u, :lens[u]] = idx[ptr[u]:ptr[u + 1]]
    pad_dev = torch.from_numpy(pad).to(dev)

    def torch_route():
        a = F.normalize(cf.index_select(0, lists[0].reshape(-1).long()).view(n, k, d), dim=2, eps=1e-8)
        h = F.normalize(cf.index_select(0, pad_dev.clamp(min=0).reshape(-1)).view(n, hmax, d), dim=2, eps=1e-8)
        s = torch.bmm(a, h.transpose(1, 2)).masked_fill((pad_dev < 0).unsqueeze(1), float("-inf"))
        sim, pos = s.topk(m, dim=2)
        return pad_dev.unsqueeze(1).expand(n, k, hmax).gather(2, pos), sim

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    routes = {"topk": topk, "explain": explain, "topk_explain": topk_explain, "explain_heavy_tail": explain_heavy,
              "torch": torch_route}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch_route()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base_mem
    times = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn))

    # agreement (module docstring)
    why_idx, why_sim, flags = explain()
    t_idx, t_sim = torch_route()
    assert not bool(flags.any()) and bool((lists[2] == k).all()) and not bool(explain_heavy()[2].any())
    same = float((t_idx == why_idx.long()).float().mean())
    tol = 2 * ((d + 15) // 16 * 16 + 8) * 2.0 ** -24
    diff = float((t_sim - why_sim).abs().max())
    agreement = {"reasons_equal_to_torch": same, "similarity_max_abs_diff": diff, "similarity_tolerance": tol}
    print("agreement: %s" % json.dumps(agreement), file=sys.stderr)
    assert same >= 0.99, same
    assert diff <= tol, (diff, tol)

    def stat(name):
        t = times[name]
        return {"median": float(np.median(t)), "min": min(t), "max": max(t)}

    def spread(name):
        return max(times[name]) - min(times[name])

    med = {name: float(np.median(t)) for name, t in times.items()}
    rows_read = n * k + int(lens.sum()) * ((k + 63) // 64)  # list rows once, history rows once per 64-row pass
    res = {
        "bench": "explain", "device": torch.cuda.get_device_name(0),
        "shape": {"n_users": n, "n_cand": n_cand, "d": d, "k": k, "reasons": m, "plays_min": lo, "plays_max": hi,
                  "plays_mean": float(lens.mean()), "score": "cosine",
                  "heavy_tail": {"users": args.heavy_users, "plays": args.heavy_plays}},
        "reps": args.reps, "warmup": args.warmup,
        "ms": {name: stat(name) for name in routes},
        "explain_share_of_topk": med["explain"] / med["topk"],
        "topk_explain_over_topk": med["topk_explain"] / med["topk"],
        "torch_over_fused": med["torch"] / med["explain"],
        "faster_beyond_noise": bool(med["torch"] - med["explain"] > max(spread("explain"), spread("torch"))),
        "heavy_tail_over_plain": med["explain_heavy_tail"] / med["explain"],
        "explain_us_per_list": med["explain"] * 1e3 / n,
        "explain_row_gather_gbps": rows_read * ((d + 15) // 16 * 16) * 4 / (med["explain"] * 1e-3) / 1e9,
        "torch_peak_bytes": int(peak),
        "fused_workspace_bytes": n_cand * ((d + 15) // 16 * 16) * 4,
        "agreement": agreement,
        "not_measured": ["kernel time by rocprofv3 (the split between k_rank_normalize and k_list_explain)",
                         "other k, d, reasons and history lengths", "masked histories",
                         "the torch route on the heavy-tail histories", "occupancy counters"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
