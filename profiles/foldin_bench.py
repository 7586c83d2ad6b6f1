"""Time the fused fold-in of unseen users (dcue_user_foldin through rank.FoldIn) against the loop a
user would write in torch today, at BASELINE config 2's shape, and print one JSON line.

  python3 profiles/foldin_bench.py [--reps 5] [--out profiles/foldin_bench.json]

Shape: seeded random towers (DCUENet's own initialisation, E = 300, d = 128), 200,000 Gaussian
candidates, 4,096 new users with about 50 plays each, N = 20 negatives per positive, max_pos = 64,
T = 30 Adam steps.
A (fused):  FoldIn.fold_in_raw -- k_rank_normalize, then ONE k_foldin launch for all 30 steps.
B (torch):  the same negatives (dcue_foldin_negatives, drawn before the clock starts) and rotating
            positives; per step a batched gather of the normalised rows [n, P, 1 + N, d], the tower and the
            hinge under autograd, torch.optim.Adam on the rows -- on the same device, in fp32.
Device events around each call, both routes warmed up, A and B alternating in one process; median and
min-max spread of each. Needs an MI355X: without a GPU it fails.

Agreement (asserted, the rule of tests/test_gpu_foldin.py): B is run once more in fp64 as the
reference; A's per-user final loss is within 50x the largest |B32 - B64| of it, under the condition
that at most 0.1 % of B64's hinge arguments lie within 1e-5 of zero.
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
    ap.add_argument("--E", type=int, default=300)
    ap.add_argument("--plays", type=int, default=50, help="mean history length (uniform in +-20)")
    ap.add_argument("--n-neg", type=int, default=20)
    ap.add_argument("--max-pos", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("foldin_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend.dcue.dcue import DCUENet
    from dcrecommend.nn import rank
    dev = torch.device("cuda:0")
    n, n_cand, d, E, N, MP, T = args.n_users, args.n_cand, args.d, args.E, args.n_neg, args.max_pos, args.steps
    margin, betas, eps = 0.2, (0.9, 0.99), 1e-8

    torch.manual_seed(args.seed)
    net = DCUENet({"feature_dim": d, "conv_hidden": 128, "user_embdim": E, "user_count": 4,
                   "model_type": "truedcuemel1dbn"}).to(dev)
    net._require_device()
    ut = net.user_embd
    W = [p.detach().clone() for p in (ut.linear1.weight, ut.linear1.bias, ut.linear2.weight, ut.linear2.bias)]
    rs = np.random.RandomState(args.seed)
    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    cf = torch.randn(n_cand, d, generator=gen).to(dev)
    init = torch.randn(n, E, generator=gen).to(dev)
    lens = rs.randint(max(1, args.plays - 20), args.plays + 21, n)
    hists = [np.sort(rs.choice(n_cand, l, replace=False)).astype(np.int32) for l in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(hists)
    fi = rank.FoldIn(None, dev, n_cand=n_cand)
    cfg = rank.FoldIn.config(T, N, MP, margin, args.lr, betas[0], betas[1], eps, 0.0, args.seed)
    model = net._model_struct()

    # B's inputs, prepared before the clock starts: per step the positives (rotating window) and the
    # kernel's own negatives; -1 marks an unused or dropped slot
    Hpad = np.zeros((n, lens.max()), np.int64)
    for r, h in enumerate(hists):
        Hpad[r, :len(h)] = h
    P = np.minimum(lens, MP)
    slot = np.arange(MP)[None, :]
    pos_t, neg_t = [], []
    for t in range(T):
        p = Hpad[np.arange(n)[:, None], (t * MP + slot) % lens[:, None]]
        pos_t.append(torch.from_numpy(np.where(slot < P[:, None], p, -1)).to(dev))
        neg_t.append(fi.negatives(ptr, idx, n, cfg, t).long())
    invP = torch.from_numpy(1.0 / P).to(dev)

    def fused():
        return fi.fold_in_raw(model, cf, ptr, idx, init, cfg)

    def baseline(dtype=torch.float32, keep=False):
        W1, b1, W2, b2 = [w.to(dtype) for w in W]
        cn = F.normalize(cf.to(dtype), dim=1, eps=1e-8)
        e = init.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([e], lr=args.lr, betas=betas, eps=eps)
        losses, near, total = [], 0, 0
        for t in range(T):
            uf = F.linear(F.relu(F.linear(F.relu(e), W1, b1)), W2, b2)
            un = F.normalize(uf, dim=1, eps=1e-8)
            pos, neg = pos_t[t], neg_t[t]
            valid = (neg >= 0) & (pos >= 0)[:, :, None]
            cpos = (cn[pos.clamp_min(0)] * un[:, None, :]).sum(-1)             # [n, MP]
            cneg = (cn[neg.clamp_min(0)] * un[:, None, None, :]).sum(-1)       # [n, MP, N]
            h = margin - (cpos[:, :, None] - cneg)
            per_user = (torch.clamp(h, min=0) * valid).sum((1, 2)) * invP.to(dtype)
            opt.zero_grad(set_to_none=True)
            per_user.sum().backward()
            opt.step()
            losses.append(per_user.detach())
            if keep:
                near += int(((h.detach().abs() < 1e-5) & valid).sum())
                total += int(valid.sum())
        return torch.stack(losses, 1), near, total

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        fused()
        baseline()
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t_f, t_b = [], []
    for _ in range(args.reps):
        t_f.append(timed(fused))
        t_b.append(timed(baseline))
    torch_peak = torch.cuda.max_memory_allocated() - base_mem

    # agreement (module docstring)
    emb, feat, loss, _, flags = fused()
    l32, _, _ = baseline()
    l64, near, total = baseline(torch.float64, keep=True)
    spread = float((l32[:, -1].double() - l64[:, -1]).abs().max())
    err = float((loss[:, -1].double() - l64[:, -1]).abs().max())
    first, last = float(loss[:, 0].mean()), float(loss[:, -1].mean())
    agreement = {"final_loss_max_err_vs_fp64": err, "torch_fp32_vs_fp64_spread": spread, "bound": 50 * spread,
                 "hinge_args_within_1e-5": near, "hinge_args": total,
                 "mean_loss_first_step": first, "mean_loss_last_step": last,
                 "rows_with_dropped_slots": int(((flags & 4) != 0).sum())}
    print("agreement: %s" % json.dumps(agreement), file=sys.stderr)
    assert not bool((flags & 3).any())
    assert near <= total // 1000, (near, total)
    assert err <= 50 * spread, (err, spread)
    assert last < first

    med_f, med_b = float(np.median(t_f)), float(np.median(t_b))
    spread_f, spread_b = max(t_f) - min(t_f), max(t_b) - min(t_b)
    rows = int((np.minimum(lens, MP) * (1 + N)).sum())  # normalised rows read per step
    res = {
        "bench": "foldin", "device": torch.cuda.get_device_name(0),
        "shape": {"n_cand": n_cand, "n_users": n, "d": d, "E": E, "n_neg": N, "max_pos": MP, "steps": T,
                  "mean_history": float(lens.mean()), "lr": args.lr},
        "reps": args.reps, "warmup": args.warmup,
        "fused_ms": {"median": med_f, "min": min(t_f), "max": max(t_f)},
        "torch_ms": {"median": med_b, "min": min(t_b), "max": max(t_b)},
        "torch_over_fused": med_b / med_f,
        "faster_beyond_noise": bool(med_b - med_f > max(spread_f, spread_b)),
        "fused_ms_per_step": med_f / T, "torch_ms_per_step": med_b / T,
        "fused_row_read_gbps": rows * d * 4 * T / (med_f * 1e-3) / 1e9,
        "fused_workspace_bytes": fi.workspace_bytes(model.dims, n, MP, N),
        "torch_peak_bytes": int(torch_peak),
        "torch_gathered_rows_bytes_per_step": rows * d * 4,
        "agreement": agreement,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
