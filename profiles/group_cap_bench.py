"""Time the per-artist cap on the device lists of dcue_topk (dcue_list_group_cap through rank.GroupCap and
TopK.topk_raw(max_per_group=)) against the route a user would write in torch today, at BASELINE config 2's
serving shape, and print one JSON line.

  python3 profiles/group_cap_bench.py [--reps 7] [--out profiles/group_cap_bench.json]

Shape: 4,096 Gaussian users x 200,000 Gaussian tracks, d = 128, cosine scores; pool 128 -> k 100, at most
2 songs per artist; 40,000 artists whose catalogue sizes follow Zipf's law (a track's artist is drawn with
probability proportional to 1 / rank).
  topk          TopK.topk_raw at k = 128 alone (the call synchronises its stream): the call the cap follows
  cap           GroupCap.cap_raw alone on the lists of a finished top-K call (ONE k_list_group_cap launch)
  mmr           Diversify.mmr_raw on the same lists, same session: the launch DESIGN 4.15 timed, for scale
  capped_1      TopK.topk_raw(max_per_group=2, cap_rounds=1): top-K + cap, no deepening
  capped_4      the same with cap_rounds=4: lists left short while their pool was full are ranked deeper
  torch cap     on the same device lists: gather of the groups, one sort by (group, position), the
                segmented rank from a running maximum of the segment starts, the keep mask, and a stable
                compaction (sort of the mask) of indices and scores, truncated to k
Device events around each call, every route warmed up, the routes alternating in one process; median and
min-max of each. Needs an MI355X: without a GPU it fails.

Agreement (asserted): the torch route's indices, score bits and counts equal the fused launch's exactly
(integer work on both sides). Also recorded: the share of lists the cap left short at pool 128, the share
still short after four rounds, and the rounds the deepening call used.

Not measured here: kernel time by rocprofv3 (a run of its own), other pools, caps and artist-size laws, dot
scores, the statistics launches (dcue_list_group_stats), and occupancy counters.
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
    ap.add_argument("--n-artists", type=int, default=40000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("group_cap_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend import _native as nat
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    n, n_cand, d, P, k, cap, n_groups = args.n_users, args.n_cand, args.d, args.pool, args.k, args.cap, args.n_artists

    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    cf = torch.randn(n_cand, d, generator=gen).to(dev)
    qf = torch.randn(n, d, generator=gen).to(dev)
    p = 1.0 / np.arange(1, n_groups + 1)
    group_np = np.random.RandomState(args.seed).choice(n_groups, n_cand, p=p / p.sum()).astype(np.int32)
    group_of = torch.from_numpy(group_np).to(dev)
    queries = np.arange(n)
    tk = rank.TopK(None, None, None, dev, n_cand=n_cand)
    gc, div = rank.GroupCap(dev), rank.Diversify(dev)

    def topk():
        return tk.topk_raw(qf, cf, queries, P)

    pool = topk()

    def cap_only():
        return gc.cap_raw(pool[0], pool[1], pool[2], group_of, n_groups, cap, k)

    def mmr():
        return div.mmr_raw(pool[0], pool[1], pool[2], cf, k, 0.7, "raw")

    def capped_1():
        return tk.topk_raw(qf, cf, queries, k, pool=P, group_of=group_np, max_per_group=cap, cap_rounds=1)

    def capped_4():
        return tk.topk_raw(qf, cf, queries, k, pool=P, group_of=group_np, max_per_group=cap, cap_rounds=4)

    pos = torch.arange(P, device=dev, dtype=torch.int64).expand(n, P)

    def torch_cap():
        idx, score = pool[0], pool[1]
        g = group_of[idx.long()].long()  # [n, P] (these pools are full: no padding to mask)
        order = torch.argsort(g * P + pos, dim=1)  # by (group, position)
        gs = g.gather(1, order)
        start = torch.ones_like(gs, dtype=torch.bool)
        start[:, 1:] = gs[:, 1:] != gs[:, :-1]
        seg = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), dim=1).values
        rank_sorted = pos - seg  # entries of the same group ahead of this one
        r = torch.empty_like(rank_sorted).scatter_(1, order, rank_sorted)
        keep = (r < cap) | (g < 0)
        front = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :k]  # survivors first, in pool order
        cnt = keep.sum(1).clamp(max=k).to(torch.int32)
        live = pos[:, :k] < cnt[:, None]
        out_idx = torch.where(live, idx.gather(1, front), torch.full_like(front, -1, dtype=torch.int32))
        out_score = torch.where(live, score.gather(1, front), torch.full_like(score[:, :k], float("-inf")))
        return out_idx, out_score, cnt

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    routes = {"topk": topk, "cap": cap_only, "mmr": mmr, "capped_1": capped_1, "capped_4": capped_4,
              "torch_cap": torch_cap}
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
    assert bool((pool[2] == P).all()) and not bool(pool[3].any())
    fused, t = cap_only(), torch_cap()
    assert torch.equal(fused[0], t[0]) and torch.equal(fused[1].view(torch.int32), t[1].view(torch.int32))
    assert torch.equal(fused[2], t[2])
    short_1 = float(((fused[4] & nat.GROUP_FLAG_SHORT) != 0).float().mean())
    deep = capped_4()
    rounds = tk.cap_rounds_used
    short_4 = float(((deep[3] & nat.GROUP_FLAG_SHORT) != 0).float().mean())
    agreement = {"torch_equals_fused": True, "lists_short_at_pool": short_1, "lists_short_after_4_rounds": short_4,
                 "rounds_used": rounds, "mean_dropped_per_list": float(fused[3].float().mean())}
    print("agreement: %s" % json.dumps(agreement), file=sys.stderr)

    def stat(name):
        v = times[name]
        return {"median": float(np.median(v)), "min": min(v), "max": max(v)}

    def spread(name):
        return max(times[name]) - min(times[name])

    med = {name: float(np.median(v)) for name, v in times.items()}
    moved = n * (P * 12 + k * 8 + 16)  # idx + score + one 4-byte group gather in, idx + score out, the per-list words
    res = {
        "bench": "group_cap", "device": torch.cuda.get_device_name(0),
        "shape": {"n_users": n, "n_cand": n_cand, "d": d, "pool": P, "k": k, "max_per_artist": cap,
                  "n_artists": n_groups, "artist_sizes": "zipf (p ~ 1 / rank)", "score": "cosine"},
        "reps": args.reps, "warmup": args.warmup,
        "ms": {name: stat(name) for name in routes},
        "cap_share_of_topk": med["cap"] / med["topk"],
        "cap_over_mmr": med["cap"] / med["mmr"],
        "capped_1_over_topk": med["capped_1"] / med["topk"],
        "capped_4_over_topk": med["capped_4"] / med["topk"],
        "torch_cap_over_fused": med["torch_cap"] / med["cap"],
        "cap_faster_beyond_noise": bool(med["torch_cap"] - med["cap"] > max(spread("cap"), spread("torch_cap"))),
        "cap_us_per_list": med["cap"] * 1e3 / n,
        "cap_bytes_moved": moved,
        "cap_gbps": moved / (med["cap"] * 1e-3) / 1e9,
        "torch_peak_bytes": int(peak),
        "fused_workspace_bytes": 0,
        "agreement": agreement,
        "not_measured": ["kernel time by rocprofv3", "other pools, caps and artist-size laws", "dot scores",
                         "the statistics launches", "occupancy counters"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
