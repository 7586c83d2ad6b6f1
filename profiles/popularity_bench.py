"""Time popularity-aware serving at BASELINE config 2's serving shape and print one JSON line.

  python3 profiles/popularity_bench.py [--parent-lib PATH/libdcue_hip.so] [--out profiles/popularity_bench.json]

Shape: seeded random factors, 200,000 candidates x d = 128, 100,000 query rows, 4,096 queries, k = 100, an
exclusion CSR of about 50 sorted items per query row (profiles/topk_bench.py's), a Gaussian prior.

1. The plain dcue_topk call, this build against the parent commit's library (--parent-lib), the two
   alternating in FRESH child processes (each loads one library through ctypes alone, warms up, and times
   `reps` calls with device events). The allowance for a difference is the parent's own spread.
2. In one process, alternating: the plain call, the prior call (dcue_topk_prior), and the torch route
   normalise, Q @ C.T + p, scatter -inf, torch.topk. Agreement of the prior call with the torch route is
   asserted as topk_bench.py asserts it, with tol widened by one rounding of the sum.
3. The statistics launches (dcue_list_item_stats + its mean, dcue_exposure_gini) on the device lists, against
   lists-to-host plus the numpy restatement (tests/popularity_reference.py), and as a share of the dcue_topk
   call they follow.
Medians with min-max. Needs an MI355X: without a GPU it fails.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from topk_bench import exclusion_csr  # noqa: E402


def _ms(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def _inputs(args, torch, dev):
    rs = np.random.RandomState(args.seed)
    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    qf = torch.randn(args.n_rows, args.d, generator=gen).to(dev)
    cf = torch.randn(args.n_cand, args.d, generator=gen).to(dev)
    queries = rs.choice(args.n_rows, args.n_queries, replace=False).astype(np.int32)
    ptr, idx = exclusion_csr(rs, args.n_rows, args.n_cand, args.excl)
    prior = (0.1 * rs.randn(args.n_cand)).astype(np.float32)
    return qf, cf, queries, ptr, idx, prior


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def child(args):
    """The plain dcue_topk call of ONE library, loaded through ctypes alone (the parent commit's has no newer
    symbol); prints {"ms": [...]}."""
    import torch
    dev = torch.device("cuda:0")
    lib = ctypes.CDLL(args.child)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.dcue_topk_workspace_bytes.argtypes = [i64, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.dcue_topk.argtypes = [P, i64, P, i64, i32, P, i32, P, P, P, i32, i32, i32, P, ctypes.c_size_t, P, P, P, P, P]
    qf, cf, queries, ptr, idx, _ = _inputs(args, torch, dev)
    nq, k = args.n_queries, args.k
    q = torch.from_numpy(queries).to(dev)
    dptr, didx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    nbytes = ctypes.c_size_t()
    assert lib.dcue_topk_workspace_bytes(args.n_cand, args.d, nq, k, 0, ctypes.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), device=dev),
           torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        st = lib.dcue_topk(qf.data_ptr(), args.n_rows, cf.data_ptr(), args.n_cand, args.d, q.data_ptr(), nq,
                           dptr.data_ptr(), didx.data_ptr(), None, k, nq, 0, ws.data_ptr(), nbytes.value,
                           *[t.data_ptr() for t in out], stream)
        assert st == 0, st

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ms = [_timed(torch, call) for _ in range(args.reps)]
    assert int(out[3].max()) == 0 and bool((out[2] == k).all())
    print(json.dumps({"ms": ms, "checksum": int(out[0].long().sum())}))
    return 0


def across_builds(args, argv):
    """{"change": ..., "parent": ...}: the plain call's times per build, children alternating."""
    from dcrecommend import _native as nat
    libs = {"change": nat.LIB_PATH, "parent": args.parent_lib}
    runs = {name: [] for name in libs}
    sums = set()
    for _ in range(args.rounds):
        for name, path in libs.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path] + argv
            res = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
                             .stdout.strip().splitlines()[-1])
            runs[name].append(res["ms"])
            sums.add(res["checksum"])
    assert len(sums) == 1, "the two builds' plain lists differ"
    out = {}
    for name, r in runs.items():
        out[name] = dict(_ms([t for run in r for t in run]), process_medians=[float(np.median(x)) for x in r])
    spread = out["parent"]["max"] - out["parent"]["min"]
    out["parent_spread_ms"] = spread
    out["median_difference_ms"] = out["change"]["median"] - out["parent"]["median"]
    out["within_parent_spread"] = bool(abs(out["median_difference_ms"]) <= spread)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-cand", type=int, default=200000)
    ap.add_argument("--n-rows", type=int, default=100000)
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--excl", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per build")
    ap.add_argument("--host-reps", type=int, default=3, help="repetitions of the lists-to-host + numpy route")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent-lib", help="the parent commit's libdcue_hip.so (part 1 is skipped without it)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    argv = sys.argv[1:] if argv is None else list(argv)
    args = ap.parse_args(argv)
    if args.child:
        return child(args)

    builds = None
    if args.parent_lib:  # (before this process opens the GPU)
        keep = [a for i, a in enumerate(argv) if a not in ("--parent-lib", "--out") and
                (i == 0 or argv[i - 1] not in ("--parent-lib", "--out"))]
        builds = across_builds(args, keep)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("popularity_bench: no GPU found (this measurement runs only on the MI355X)")
    import popularity_reference as R
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    n_cand, n_rows, nq, d, k = args.n_cand, args.n_rows, args.n_queries, args.d, args.k
    dp = (d + 15) // 16 * 16
    qf, cf, queries, ptr, idx, prior = _inputs(args, torch, dev)
    tol = (dp + 8) * 2.0 ** -24 + 2.0 ** -24 * (1.0 + float(np.abs(prior).max()))
    tk = rank.TopK(ptr, idx, None, dev, n_cand=n_cand)
    lens = (ptr[queries.astype(np.int64) + 1] - ptr[queries]).astype(np.int64)
    ex_rows = torch.from_numpy(np.repeat(np.arange(nq, dtype=np.int64), lens)).to(dev)
    ex_cols = torch.from_numpy(np.concatenate([idx[ptr[q]:ptr[q + 1]] for q in queries]).astype(np.int64)).to(dev)
    q_dev = torch.from_numpy(queries.astype(np.int64)).to(dev)
    p_dev = torch.from_numpy(prior).to(dev)

    def plain():
        return tk.topk_raw(qf, cf, queries, k)

    def with_prior():
        return tk.topk_raw(qf, cf, queries, k, prior=prior)

    def torch_route(keep=False):
        qn = qf.index_select(0, q_dev)
        qn = qn / qn.norm(dim=1, keepdim=True).clamp_min(1e-8)
        cn = cf / cf.norm(dim=1, keepdim=True).clamp_min(1e-8)
        S = qn @ cn.t() + p_dev
        S[ex_rows, ex_cols] = float("-inf")
        val, ind = torch.topk(S, k, dim=1)
        return (val, ind, S) if keep else (val, ind)

    for _ in range(args.warmup):
        plain(), with_prior(), torch_route()
    torch.cuda.synchronize()
    t_plain, t_prior, t_torch = [], [], []
    for _ in range(args.reps):
        t_plain.append(_timed(torch, plain))
        t_prior.append(_timed(torch, with_prior))
        t_torch.append(_timed(torch, torch_route))

    # agreement of the prior call with the torch route (topk_bench.py's assertions)
    f_idx, f_score, f_count, f_flags = with_prior()
    val, ind, S = torch_route(keep=True)
    f_idx = f_idx.long()
    assert int(f_flags.max()) == 0 and bool((f_count == k).all())
    srt = f_idx.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "repeated index in a fused row"
    at = S.gather(1, f_idx)
    assert bool(torch.isfinite(at).all()), "the fused path returned an excluded item"
    score_err = float((at - f_score).abs().max())
    assert score_err <= 2 * tol, score_err
    t = val[:, k - 1:k]
    assert bool((at >= t - 4 * tol).all()), "the fused path returned an item from below the k-th score"
    assert bool(((S > t + 4 * tol).sum(1) == (at > t + 4 * tol).sum(1)).all()), "the fused path missed an item"
    same = float((f_idx == ind).float().mean())
    del S, at

    # the statistics launches on the prior call's device lists
    ks = (10, 50, 100)
    rs = np.random.RandomState(args.seed + 1)
    counts = rs.zipf(1.5, n_cand).astype(np.int64)
    from dcrecommend.datasets import popularity as H
    value, tail = H.self_information(counts), H.tail_bytes(counts)
    pop = rank.PopStats(dev, n_cand, value, tail)
    truth_ptr = np.arange(n_rows + 1, dtype=np.int64)
    ev = rank.TopKMetrics(truth_ptr, np.zeros(n_rows, np.int32), dev, n_cand=n_cand)
    lists, _, count, _ = with_prior()
    exposure = ev.new_exposure(len(ks))
    ev.metrics_raw(lists, count, queries, ks, exposure=exposure)

    def device_stats():
        st, fl = pop.stats_raw(lists, count, ks)
        mean, _ = pop.mean_raw(st, fl)
        g, _ = pop.gini_raw(exposure, nq)
        return mean, g

    def host_stats():
        li, co, ex = lists.cpu().numpy(), count.cpu().numpy(), exposure.cpu().numpy()
        st, fl = R.item_stats(li, co, list(ks), value, tail, n_cand)
        return R.col_mean(st.reshape(len(li), -1), fl)[0], R.gini(ex)[0]

    for _ in range(args.warmup):
        device_stats()
    torch.cuda.synchronize()
    t_dev = [_timed(torch, device_stats) for _ in range(args.reps)]
    t_host = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        want = host_stats()
        t_host.append((time.perf_counter() - t0) * 1e3)
    got = device_stats()
    assert np.array_equal(got[0].cpu().numpy().reshape(-1).view(np.uint64), want[0].view(np.uint64)), "item stats differ"
    assert np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1].view(np.uint64)), "Gini differs"

    med = {n: float(np.median(x)) for n, x in (("plain", t_plain), ("prior", t_prior), ("torch", t_torch), ("stats", t_dev))}
    res = {
        "bench": "popularity", "device": torch.cuda.get_device_name(0),
        "shape": {"n_cand": n_cand, "n_query_rows": n_rows, "n_queries": nq, "d": d, "k": k,
                  "excluded_items": int(ex_cols.numel()), "cutoffs": list(ks)},
        "reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps,
        "plain_across_builds_ms": builds,
        "plain_ms": _ms(t_plain), "prior_ms": _ms(t_prior), "torch_ms": _ms(t_torch),
        "prior_minus_plain_ms": med["prior"] - med["plain"],
        "prior_over_plain": med["prior"] / med["plain"],
        "torch_over_prior": med["torch"] / med["prior"],
        "agreement": {"tol": tol, "max_score_diff": score_err, "positions_identical": same},
        "stats_device_ms": _ms(t_dev), "stats_host_ms": _ms(t_host),
        "stats_host_over_device": float(np.median(t_host)) / med["stats"],
        "stats_share_of_topk_call": med["stats"] / med["prior"],
        "novelty_mean_bits": [float(x) for x in got[0].cpu().numpy()[:, 0]],
        "gini": [float(x) for x in got[1].cpu().numpy()],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
