"""numpy fp64 restatement of dcue_topk_metrics / dcue_topk_metrics_mean (include/dcue.h), in plain
loops: the six per-query metrics at each cutoff, the flags, the exposure counts and coverage, and
the means over the evaluated queries. The GPU tests and profiles/topk_metrics_bench.py compare
against it; the reference project has no counterpart."""
import math

import numpy as np

N_METRICS = 6
PRECISION, RECALL, NDCG, MAP, MRR, HIT = range(N_METRICS)
NAMES = ("precision", "recall", "ndcg", "map", "mrr", "hit")
FLAG_NO_TRUTH, FLAG_BAD_INDEX = 1, 2


def query_metrics(lst, c, truth, ks):
    """[len(ks)][6] for one query: lst the list (only lst[:c] is looked at), truth the set T (not
    empty), ks ascending cutoffs."""
    truth = set(int(x) for x in truth)
    t = len(truth)
    out = np.zeros((len(ks), N_METRICS), np.float64)
    for i, kap in enumerate(ks):
        hits, dcg, ap, first = 0, 0.0, 0.0, None
        for j in range(kap):
            if j < c and int(lst[j]) in truth:
                hits += 1
                dcg += 1.0 / math.log2(j + 2)
                ap += hits / (j + 1)
                if first is None:
                    first = j
        idcg = 0.0
        for j in range(min(kap, t)):
            idcg += 1.0 / math.log2(j + 2)
        out[i] = (hits / kap, hits / t, dcg / idcg, ap / min(kap, t), 0.0 if first is None else 1.0 / (first + 1),
                  1.0 if hits else 0.0)
    return out


def metrics(idx, count, queries, truth_ptr, truth_idx, ks, n_cand, exposure=None):
    """(metrics [n][m][6], flags [n]) for lists idx [n][k] / count [n] of query rows `queries`;
    accumulates into exposure int64 [m][n_cand] when given. Flag bit 0: empty truth row; bit 1: an
    entry before `count` outside [0, n_cand). A flagged query's metrics are 0 and it adds no exposure."""
    idx = np.asarray(idx)
    n, k = idx.shape
    out = np.zeros((n, len(ks), N_METRICS), np.float64)
    flags = np.zeros(n, np.int32)
    for q in range(n):
        row = int(queries[q])
        truth = truth_idx[truth_ptr[row]:truth_ptr[row + 1]]
        c = min(max(int(count[q]), 0), k)
        lst = idx[q]
        if len(truth) == 0:
            flags[q] |= FLAG_NO_TRUTH
        if any(int(x) < 0 or int(x) >= n_cand for x in lst[:c]):
            flags[q] |= FLAG_BAD_INDEX
        if flags[q]:
            continue
        out[q] = query_metrics(lst, c, truth, ks)
        if exposure is not None:
            for j in range(min(c, ks[-1])):
                i = next(i for i, kap in enumerate(ks) if j < kap)
                exposure[i, int(lst[j])] += 1
    return out, flags


def means(per_query, flags):
    """(mean [m][6] over the queries with flags == 0, their number); zeros when there is none."""
    keep = np.asarray(flags) == 0
    if not keep.any():
        return np.zeros(per_query.shape[1:], np.float64), 0
    return np.mean(np.asarray(per_query, np.float64)[keep], axis=0), int(keep.sum())


def coverage(exposure, cand_mask, n_cand):
    """[m]: distinct candidates among the first ks[i] entries of any evaluated query, over the
    candidates with a non-zero mask byte (n_cand without a mask)."""
    denom = int(np.count_nonzero(cand_mask)) if cand_mask is not None else int(n_cand)
    seen = np.zeros(exposure.shape[1], bool)
    out = np.zeros(exposure.shape[0], np.float64)
    for i in range(exposure.shape[0]):
        seen |= exposure[i] != 0
        out[i] = (int(seen.sum()) / denom) if denom else 0.0
    return out
