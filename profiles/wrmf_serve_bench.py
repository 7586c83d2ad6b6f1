"""Time the WRMF serving path at BASELINE config 2's shape and print one JSON line.

  python3 profiles/wrmf_serve_bench.py [--out profiles/wrmf_serve_bench.json]

Shape: 100,000 users x 200,000 items, d = 128, 5,000,000 seeded random pairs with play counts, item
factors with log-normal row norms (so that the inner product and the cosine rank differently).

1. Top-100 for 4,096 users: the inner-product call (rank.TopK(score="dot"), dcue_topk_scored) against the
   cosine call (dcue_topk) on the same inputs -- the same score kernel behind a cheaper prep pass, so
   parity is expected -- alternating, `--runs` each after a warm-up; and the torch route a user would
   write: Q @ C.T, scatter -inf over the exclusions, torch.topk. A control repeats dot against cosine on
   item factors WITHOUT the log-normal norms (every row norm about the same), to tell what the score
   mode costs from what these inputs cost.
2. The objective: WRMF.objective_terms (dcue_wrmf_objective) against a torch restatement of the same
   identity (a gathered fp64 pair dot over the CSR in chunks, plus two fp64 Grams). Its bound is the
   gather, nnz x d x 4 bytes of item rows, over the measured HBM rate (6.29 TB/s).
3. WRMF.fold_in of 4,096 histories of about 50 items (host CSR build included).

Host clock around calls that end in a device synchronise. Needs an MI355X: without a GPU it fails.
Agreement (asserted): the dot lists against the torch score matrix as in profiles/topk_bench.py with
tol = 1.01 d 2^-24 |q| max |c|; the objective against the torch restatement to 1e-9 relative.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))

HBM_MEASURED_TBS = 6.29


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-users", type=int, default=100000)
    ap.add_argument("--n-items", type=int, default=200000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nnz", type=int, default=5000000)
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--history", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wrmf_serve_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend.dcbr import WRMF, device_csr
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    nu, ni, d, nq, k = args.n_users, args.n_items, args.d, args.n_queries, args.k
    alpha, lam = 40.0, 0.01

    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    rs = np.random.RandomState(args.seed)
    m = WRMF(factors=d, regularization=lam, alpha=alpha, iterations=0, device=dev)
    u = torch.randint(0, nu, (args.nnz,), generator=gen).to(dev)
    i = torch.randint(0, ni, (args.nnz,), generator=gen).to(dev)
    key = torch.unique(u * ni + i)  # distinct pairs, sorted by user then item
    u, i = key // ni, key % ni
    v = torch.randint(1, 21, (key.numel(),), generator=gen).float().to(dev)
    m.by_user = device_csr(u, i, v, nu)
    m.by_item = device_csr(i, u, v, ni)
    m.init_factors(nu, ni)
    m.user_factors.copy_((torch.randn(nu, d, generator=gen) * 0.1).to(dev))
    y_plain = (torch.randn(ni, d, generator=gen) * 0.1).to(dev)  # the control's candidates: no norm spread
    m.item_factors.copy_(y_plain * torch.exp(0.5 * torch.randn(ni, 1, generator=gen)).to(dev))
    nnz = int(key.numel())
    X, Y = m.user_factors, m.item_factors
    queries = rs.choice(nu, nq, replace=False).astype(np.int64)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(ts):
        return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}

    # ---- 1. top-K
    ptr, idx = m._seen()
    tk_dot = rank.TopK(ptr, idx, None, dev, n_cand=ni, score="dot")
    tk_cos = rank.TopK(ptr, idx, None, dev, n_cand=ni)
    q_dev = torch.from_numpy(queries).to(dev)
    lens = (ptr[q_dev + 1] - ptr[q_dev])
    ex_rows = torch.repeat_interleave(torch.arange(nq, device=dev), lens)
    starts = ptr[q_dev]
    offs = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    ex_cols = idx[torch.repeat_interleave(starts, lens) + offs].long()

    def dot():
        return tk_dot.topk_raw(X, Y, queries, k)

    def cos():
        return tk_cos.topk_raw(X, Y, queries, k)

    def torch_route(keep=False):
        S = X.index_select(0, q_dev) @ Y.t()
        S[ex_rows, ex_cols] = float("-inf")
        val, ind = torch.topk(S, k, dim=1)
        return (val, ind, S) if keep else (val, ind)

    for _ in range(args.warmup):
        dot(), cos(), torch_route()
    t_dot, t_cos, t_torch = [], [], []
    for _ in range(args.runs):
        t_dot.append(wall(dot)[0])
        t_cos.append(wall(cos)[0])
    for _ in range(args.runs):
        t_torch.append(wall(torch_route)[0])
    f_idx, f_score, f_count, f_flags = dot()
    val, ind, S = torch_route(keep=True)
    f_idx = f_idx.long()
    assert int(f_flags.max()) == 0 and bool((f_count == k).all())
    tol = (1.01 * d * 2.0 ** -24 * X.index_select(0, q_dev).double().norm(dim=1) * Y.double().norm(dim=1).max())
    tol = tol.float().unsqueeze(1)
    at = S.gather(1, f_idx)
    assert bool(torch.isfinite(at).all()), "the dot path returned an excluded item"
    score_err = float(((at - f_score).abs() / tol).max())
    assert score_err <= 2.0, score_err
    t = val[:, k - 1:k]
    assert bool((at >= t - 4 * tol).all()), "the dot path returned an item from below the k-th score"
    assert bool(((S > t + 4 * tol).sum(1) == (at > t + 4 * tol).sum(1)).all()), "the dot path missed an item"
    same = float((f_idx == ind).float().mean())
    c_idx = cos()[0].long()
    shared = float(np.mean([len(np.intersect1d(a, b)) for a, b in zip(f_idx[:256].cpu().numpy(), c_idx[:256].cpu().numpy())]) / k)
    del S, at
    spread = max(max(t_dot) - min(t_dot), max(t_cos) - min(t_cos))
    # the control: the same two calls on candidates of about equal norm
    for _ in range(args.warmup):
        tk_dot.topk_raw(X, y_plain, queries, k), tk_cos.topk_raw(X, y_plain, queries, k)
    c_dot, c_cos = [], []
    for _ in range(args.runs):
        c_dot.append(wall(lambda: tk_dot.topk_raw(X, y_plain, queries, k))[0])
        c_cos.append(wall(lambda: tk_cos.topk_raw(X, y_plain, queries, k))[0])

    # ---- 2. the objective
    indptr, indices, values = m.by_user
    rows = torch.repeat_interleave(torch.arange(nu, device=dev), indptr[1:] - indptr[:-1])

    def torch_objective(chunk=1 << 20):
        obs = torch.zeros((), dtype=torch.float64, device=dev)
        for a in range(0, nnz, chunk):
            s = (X[rows[a:a + chunk]].double() * Y[indices[a:a + chunk].long()].double()).sum(1)
            c = 1.0 + alpha * values[a:a + chunk].double()
            obs += (c * (1.0 - s) ** 2 - s * s).sum()
        gx, gy = X.double().t() @ X.double(), Y.double().t() @ Y.double()
        return float(obs + (gx * gy).sum() + lam * (torch.trace(gx) + torch.trace(gy)))

    for _ in range(args.warmup):
        m.objective_terms(), torch_objective()
    t_obj, t_tobj = [], []
    for _ in range(args.runs):
        ms, terms = wall(m.objective_terms)
        t_obj.append(ms)
        ms, ref = wall(torch_objective)
        t_tobj.append(ms)
    obj_rel = abs(terms[0] - ref) / abs(ref)
    assert obj_rel <= 1e-9, obj_rel
    assert m.objective_terms() == terms, "two objective calls differ"
    gather_bytes = nnz * d * 4
    bound_ms = gather_bytes / (HBM_MEASURED_TBS * 1e12) * 1e3

    # ---- 3. fold-in
    hist = [np.unique(rs.randint(0, ni, rs.randint(args.history - 10, args.history + 11))) for _ in range(nq)]
    for _ in range(args.warmup):
        m.fold_in(hist)
    t_fold = [wall(lambda: m.fold_in(hist))[0] for _ in range(args.runs)]

    res = {
        "bench": "wrmf_serve", "device": torch.cuda.get_device_name(0),
        "shape": {"n_users": nu, "n_items": ni, "d": d, "pairs": nnz, "n_queries": nq, "k": k,
                  "fold_in_histories": nq, "fold_in_items": int(sum(len(h) for h in hist))},
        "runs": args.runs, "warmup": args.warmup,
        "topk_dot_ms": stats(t_dot), "topk_cosine_ms": stats(t_cos), "topk_torch_ms": stats(t_torch),
        "dot_over_cosine": float(np.median(t_dot) / np.median(t_cos)),
        "dot_minus_cosine_ms": float(np.median(t_dot) - np.median(t_cos)), "runs_spread_ms": float(spread),
        "dot_slower_beyond_spread": bool(np.median(t_dot) - np.median(t_cos) > spread),
        "torch_over_dot": float(np.median(t_torch) / np.median(t_dot)),
        "equal_norm_control": {"topk_dot_ms": stats(c_dot), "topk_cosine_ms": stats(c_cos),
                               "dot_over_cosine": float(np.median(c_dot) / np.median(c_cos))},
        "topk_agreement": {"max_score_diff_over_tol": score_err, "positions_identical_to_torch": same,
                           "entries_shared_with_cosine_list": shared},
        "objective_ms": stats(t_obj), "objective_torch_ms": stats(t_tobj),
        "torch_over_objective": float(np.median(t_tobj) / np.median(t_obj)),
        "objective_gather_bytes": gather_bytes, "objective_gather_bound_ms": bound_ms,
        "objective_share_of_gather_bound": float(bound_ms / np.median(t_obj)),
        "objective_terms": list(terms), "objective_rel_diff_to_torch": obj_rel,
        "fold_in_ms": stats(t_fold),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
