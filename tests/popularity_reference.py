"""numpy / Python restatements of popularity-aware serving (include/dcue.h dcue_topk_prior,
dcue_list_item_stats, dcue_exposure_gini; dcrecommend.datasets.popularity): the contract the GPU tests
hold the library to, written as plainly as the definitions read."""
import math

import numpy as np

import topk_reference as T


def prior_scores(s0, prior):
    """fl32(s0 + p) per pair, -0 folded to +0 on both sides of the addition: s0 float32 [n, n_cand] (the
    scores dcue_topk_scored produces), prior float32 [n_cand]."""
    s0 = np.asarray(s0, np.float32) + np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        return (s0 + np.asarray(prior, np.float32)[None, :]).astype(np.float32) + np.float32(0.0)


def topk_prior(s0, prior, queries, k, excl_ptr=None, excl_idx=None, cand_mask=None):
    """(idx [n, k] int64, score [n, k] float32, count [n], flagged [n] bool): topk_reference.select on the
    summed scores. A non-finite sum of an eligible candidate flags the query; a NaN is never selected."""
    s = prior_scores(s0, prior)
    idx, score, count, flagged = [], [], [], []
    for i, q in enumerate(queries):
        seen = T.eligible(np.zeros(s.shape[1]), int(q), excl_ptr, excl_idx, cand_mask)  # mask and exclusion only
        flagged.append(bool((~np.isfinite(s[i]) & seen).any()))
        a, b, c = T.select(s[i].astype(np.float64), T.eligible(s[i], int(q), excl_ptr, excl_idx, cand_mask), k)
        idx.append(a)
        score.append(b.astype(np.float32))
        count.append(c)
    return np.stack(idx), np.stack(score), np.array(count, np.int32), np.array(flagged)


def item_stats(idx, count, ks, item_value, item_tail, n_cand):
    """(stats float64 [n, m, 2], flags int32 [n]): sequential loops over each list's first min(K, c) entries."""
    n, k = idx.shape
    out = np.zeros((n, len(ks), 2), np.float64)
    flags = np.zeros(n, np.int32)
    for i in range(n):
        c = min(max(int(count[i]), 0), k)
        L = [int(v) for v in idx[i, :c]]
        if c == 0:
            flags[i] |= 1
        if any(v < 0 or v >= n_cand for v in L):
            flags[i] |= 2
        if flags[i]:
            continue
        for t, K in enumerate(ks):
            nk = min(K, c)
            s = np.float64(0.0)
            tails = 0
            for j in range(nk):
                if item_value is not None:
                    s = s + np.float64(item_value[L[j]])
                if item_tail is not None and item_tail[L[j]]:
                    tails += 1
            out[i, t, 0] = s / np.float64(nk)
            out[i, t, 1] = np.float64(tails) / np.float64(nk)
    return out, flags


def col_mean(values, flags, threads=1024):
    """dcue_topk_metrics_mean's fixed order over the unflagged rows of values [n, cols]: G = threads // cols
    row groups, group g adds rows g, g + G, ... in order (a flagged row adds +0), the G partials are added in
    ascending g; then one division by the number of unflagged rows."""
    values = np.asarray(values, np.float64).reshape(len(flags), -1)
    n, cols = values.shape
    G = threads // cols
    mean = np.zeros(cols, np.float64)
    ne = int((np.asarray(flags) == 0).sum())
    for col in range(cols):
        tot = np.float64(0.0)
        for g in range(G):
            s = np.float64(0.0)
            for r in range(g, n, G):
                s = s + (np.float64(0.0) if flags[r] else values[r, col])
            tot = tot + s
        mean[col] = tot / np.float64(ne) if ne else 0.0
    return mean, ne


def gini(exposure, cand_mask=None):
    """(gini float64 [m], total [m]) from a sort, in Python integers: for cutoff i over the admitted
    candidates, x = exposure[0..i] summed, G = (sum_j (2j - n - 1) x_(j)) / (n sum x), j = 1..n ascending."""
    exposure = np.asarray(exposure, np.int64)
    keep = np.ones(exposure.shape[1], bool) if cand_mask is None else np.asarray(cand_mask) != 0
    out, totals = [], []
    for i in range(exposure.shape[0]):
        x = sorted(int(v) for v in exposure[:i + 1].sum(0)[keep])
        n, total = len(x), sum(x)
        num = sum((2 * (j + 1) - n - 1) * v for j, v in enumerate(x))
        out.append(float(np.float64(num) / np.float64(n * total)) if n and total else 0.0)
        totals.append(total)
    return np.array(out, np.float64), np.array(totals, np.int64)


def gini_brute(x):
    """The mean-absolute-difference form, sum_ij |x_i - x_j| / (2 n sum x), as an exact fraction (num, den)."""
    x = [int(v) for v in x]
    return sum(abs(a - b) for a in x for b in x), 2 * len(x) * sum(x)


def log_popularity(counts):
    top = max(counts) if len(counts) else 0
    return np.array([math.log2(1 + c) / math.log2(1 + top) if top else 0.0 for c in counts], np.float64)


def self_information(counts):
    total = sum(int(c) + 1 for c in counts)
    return np.array([-math.log2((int(c) + 1) / total) for c in counts], np.float64)


def tail_bytes(counts, head_mass=0.8):
    order = sorted(range(len(counts)), key=lambda i: (-int(counts[i]), i))
    total = sum(int(c) for c in counts)
    tail = np.ones(len(counts), np.uint8)
    held = 0
    for i in order:
        if held >= head_mass * total:
            break
        tail[i] = 0
        held += int(counts[i])
    return tail
