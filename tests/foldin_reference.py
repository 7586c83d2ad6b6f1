"""Reference of the fold-in of unseen users (include/dcue.h dcue_user_foldin): a torch restatement of
the header's semantics, parameterised by dtype (fp64: the yardstick; fp32: the spread a correct fp32
implementation may show), with the integer sampler in plain Python. Shared by tests/test_foldin_cpu.py
(self-checks) and tests/test_gpu_foldin.py (the kernel against it).

Per global row r = row0 + local row, H its sorted history, P = min(|H|, max_pos), step t:
  positives   H[(t * max_pos + i) mod |H|], i < P
  negatives   mix = splitmix64 finaliser; z0 = mix(seed + 0x9E3779B97F4A7C15 (r + 1)); attempt a = 0..7:
              x = mix(z0 ^ (t << 40 | i << 24 | j << 8 | a)), c = ((x >> 32) n_cand) >> 32; the first c the
              mask admits and H does not hold; none: the slot is dropped (-1)
  loss_t      (1/P) sum_i sum_j max(0, margin - (cos(uf, f_pos_i) - cos(uf, f_neg_ij))),
              uf = W2 relu(W1 relu(e) + b1) + b2, cos = F.cosine_similarity(eps=1e-8)
  update      torch.optim.Adam on e alone (step count t + 1, constant lr, moments from 0)
"""
import bisect
import functools

import numpy as np
import torch
import torch.nn.functional as F

M64 = (1 << 64) - 1
EMPTY, NONFINITE, DROPPED = 1, 2, 4


def mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def row_key(seed, r):
    return mix((seed + 0x9E3779B97F4A7C15 * (r + 1)) & M64)


def negative(z0, t, i, j, n_cand, mask, hist):
    """hist: a sorted list. The candidate, or -1 when all eight attempts are rejected."""
    base = (t << 40) | (i << 24) | (j << 8)
    for a in range(8):
        x = mix(z0 ^ (base | a))
        c = ((x >> 32) * n_cand) >> 32
        if mask is not None and not mask[c]:
            continue
        k = bisect.bisect_left(hist, c)
        if k < len(hist) and hist[k] == c:
            continue
        return c
    return -1


def negatives(seed, r, t, hist, max_pos, n_neg, n_cand, mask):
    """int32 [max_pos, n_neg] as dcue_foldin_negatives writes row r: -1 for dropped slots and i >= P."""
    hist = [int(h) for h in hist]
    out = np.full((max_pos, n_neg), -1, np.int32)
    z0 = row_key(seed, r)
    for i in range(min(len(hist), max_pos)):
        for j in range(n_neg):
            out[i, j] = negative(z0, t, i, j, n_cand, mask, hist)
    return out


def positives(hist, t, max_pos):
    n = len(hist)
    return [int(hist[(t * max_pos + i) % n]) for i in range(min(n, max_pos))]


def tower(e, W1, b1, W2, b2):
    return F.linear(F.relu(F.linear(F.relu(e), W1, b1)), W2, b2)


def fold_in(weights, cand, mask, hists, init, steps, n_neg, max_pos, margin, lr, beta1=0.9, beta2=0.99,
            eps=1e-8, weight_decay=0.0, seed=0, row0=0, dtype=torch.float64):
    """hists[r]: the sorted history of GLOBAL row r; init [n, E]: local rows 0..n-1 = global rows
    row0.. . Returns a dict: emb [n, E], feat [n, d], loss [n, steps], grad [n, E] (the last executed
    step's gradient, before its update), flags [n], hinge (every hinge argument
    margin - (cos_pos - cos_neg) of every step, one flat array: the near-tie condition of the tests)."""
    W1, b1, W2, b2 = [torch.as_tensor(np.asarray(w)).to(dtype) for w in weights]
    cand_t = torch.as_tensor(np.asarray(cand)).to(dtype)
    n = len(init)
    E = W1.shape[1]
    emb = torch.as_tensor(np.asarray(init)).to(dtype).clone()
    loss = torch.zeros(n, steps, dtype=dtype)
    grad = torch.zeros(n, E, dtype=dtype)
    flags = np.zeros(n, np.int32)
    hinge = []
    n_cand = len(cand)
    for u in range(n):
        r = row0 + u
        hist = [int(h) for h in hists[r]]
        if not hist:
            flags[u] |= EMPTY
            continue
        z0 = row_key(seed, r)
        e = emb[u].clone().requires_grad_(True)
        m = torch.zeros(E, dtype=dtype)
        v = torch.zeros(E, dtype=dtype)
        for t in range(steps):
            pos = positives(hist, t, max_pos)
            P = len(pos)
            neg = np.array([[negative(z0, t, i, j, n_cand, mask, hist) for j in range(n_neg)] for i in range(P)])
            valid = torch.as_tensor(neg >= 0)
            if not bool(valid.all()):
                flags[u] |= DROPPED
            uf = tower(e, W1, b1, W2, b2)
            fpos = cand_t[torch.as_tensor(pos)]
            fneg = cand_t[torch.as_tensor(np.where(neg >= 0, neg, 0))]
            cpos = F.cosine_similarity(uf[None, :], fpos, dim=1, eps=1e-8)
            cneg = F.cosine_similarity(uf[None, None, :], fneg, dim=2, eps=1e-8)
            h = margin - (cpos[:, None] - cneg)
            hinge.append(h.detach()[valid].double().numpy())
            lt = (torch.maximum(torch.zeros_like(h), h) * valid.to(dtype)).sum() / P
            g, = torch.autograd.grad(lt, e)
            loss[u, t] = lt.detach()
            grad[u] = g
            with torch.no_grad():
                if weight_decay != 0:
                    g = g + weight_decay * e
                m = beta1 * m + (1 - beta1) * g
                v = beta2 * v + (1 - beta2) * g * g
                bc1 = 1 - beta1 ** (t + 1)
                bc2 = 1 - beta2 ** (t + 1)
                e -= (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
        emb[u] = e.detach()
    with torch.no_grad():
        feat = tower(emb, W1, b1, W2, b2)
    if not bool(torch.isfinite(loss).all()) or not bool(torch.isfinite(feat).all()):
        flags[(~torch.isfinite(loss).all(dim=1) | ~torch.isfinite(feat).all(dim=1)).numpy()] |= NONFINITE
    return dict(emb=emb.numpy(), feat=feat.numpy(), loss=loss.numpy(), grad=grad.numpy(), flags=flags,
                hinge=np.concatenate(hinge) if hinge else np.zeros(0))


# ------------------------------------------------------------------------------- the tests' cases
def csr(hists):
    ptr = np.zeros(len(hists) + 1, np.int64)
    for r, h in enumerate(hists):
        ptr[r + 1] = ptr[r] + len(h)
    idx = np.concatenate([np.asarray(h, np.int32) for h in hists]) if len(hists) else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def make_case(E, d, n_cand, hist_lens, seed):
    """Random towers built as DCUENet builds them (the net itself is returned for the GPU tests to
    move to the device), Gaussian candidates, a 0.8 mask, sorted random histories of the given
    lengths drawn from the admitted candidates, N(0, 1) initial rows."""
    from dcrecommend.dcue.dcue import DCUENet
    torch.manual_seed(seed)
    net = DCUENet({"feature_dim": d, "conv_hidden": 32, "user_embdim": E, "user_count": 4,
                   "model_type": "truedcuemel1d"})
    ut = net.user_embd
    weights = tuple(p.detach().clone().numpy() for p in (ut.linear1.weight, ut.linear1.bias, ut.linear2.weight,
                                                         ut.linear2.bias))
    rs = np.random.RandomState(seed)
    cand = rs.randn(n_cand, d).astype(np.float32)
    mask = (rs.rand(n_cand) < 0.8).astype(np.uint8)
    ok = np.flatnonzero(mask)
    hists = tuple(tuple(int(x) for x in np.sort(rs.choice(ok, n, replace=False))) for n in hist_lens)
    init = rs.randn(len(hist_lens), E).astype(np.float32)
    return dict(net=net, weights=weights, cand=cand, mask=mask, hists=hists, init=init, E=E, d=d)


# One step (tests 2 / 3): (E, d, n_cand, n_neg, seed) with history lengths ONE_STEP_LENS at max_pos 64;
# thirty steps (test 4): the same tuple with THIRTY_LENS at max_pos 16. Seeds chosen so that the fp64
# reference has no hinge argument within 1e-5 of zero (one step) / at most 0.1 % (thirty steps):
# tests/test_foldin_cpu.py asserts it for every case, the GPU tests again for the case they run.
ONE_STEP_LENS = (1, 5, 17, 64, 65, 200)
ONE_STEP_CASES = [(40, 32, 600, 5, 1), (40, 100, 1000, 1, 1), (40, 128, 2500, 20, 1), (40, 256, 800, 5, 1),
                  (300, 32, 600, 5, 1), (300, 100, 1000, 1, 1), (300, 128, 2500, 20, 2), (300, 256, 800, 5, 1)]
ONE_STEP_CFG = dict(steps=1, max_pos=64, margin=0.2, lr=0.05)
# beyond E = 384 .. 432 (by d) the kernel keeps m and v, beyond E = 656 .. 720 every activation in the
# workspace; an E that is no multiple of 4 reads the weight rows element by element. Here: LDS and odd E
# (401), m / v in the workspace (512, and 673 odd), everything in the workspace (801 odd, 1024)
TIER_CASES = [(401, 100, 700, 5, 1), (512, 64, 700, 5, 1), (673, 32, 700, 5, 1), (801, 32, 700, 5, 1),
              (1024, 256, 900, 5, 1)]
THIRTY_LENS = (1, 5, 17, 40, 64, 33)
THIRTY_CASES = [(40, 32, 600, 5, 1), (300, 128, 1500, 5, 1)]
THIRTY_CFG = dict(steps=30, max_pos=16, margin=0.2, lr=0.05)
NEAR_TIE = 1e-5


def reference(c, dtype, **cfg):
    """fold_in over every row of a make_case() case (cached per case object, dtype and config)."""
    key = (dtype, tuple(sorted(cfg.items())))
    cache = c.setdefault("_ref", {})
    if key not in cache:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)  # thousands of tiny ops: a thread pool only adds its hand-over time
        try:
            cache[key] = fold_in(c["weights"], c["cand"], c["mask"], c["hists"], c["init"], dtype=dtype, **cfg)
        finally:
            torch.set_num_threads(threads)
    return cache[key]


def spread(r32, r64):
    """The fp32-vs-fp64 spread of the reference on one case: max |loss32 - loss64|, and the largest
    gradient difference relative to its row's largest |g|."""
    dl = float(np.abs(r32["loss"].astype(np.float64) - r64["loss"]).max()) if r64["loss"].size else 0.0
    gmax = np.abs(r64["grad"]).max(axis=1)
    on = gmax > 0
    dg = float((np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max(axis=1)[on] / gmax[on]).max()) if on.any() else 0.0
    return dl, dg
