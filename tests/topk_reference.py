"""numpy reference of dcue_topk's selection (include/dcue.h): fp64 cosines with nn.CosineSimilarity's
1e-8 norm clamp, the eligibility rule (mask, exclusion row, not NaN) and the order -- score
descending, then candidate index ascending -- plus the tolerant comparison the GPU tests and
profiles/topk_bench.py use where fp32 scores may order near-ties differently."""
import numpy as np


def cosines(query_feat, cand_feat, queries):
    """[len(queries)][n_cand] fp64: x / max(||x||, 1e-8) on both sides, then the dot product."""
    q = np.asarray(query_feat, np.float64)[np.asarray(queries)]
    c = np.asarray(cand_feat, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), 1e-8)
        c = c / np.maximum(np.sqrt((c * c).sum(1, keepdims=True)), 1e-8)
        return q @ c.T


def eligible(scores_row, row, excl_ptr, excl_idx, cand_mask):
    """Boolean [n_cand]: mask byte non-zero, not in the query row's exclusion list, score not NaN."""
    ok = ~np.isnan(scores_row)
    if cand_mask is not None:
        ok &= np.asarray(cand_mask) != 0
    if excl_ptr is not None:
        ok[excl_idx[excl_ptr[row]:excl_ptr[row + 1]]] = False
    return ok


def select(scores_row, ok, k):
    """(idx [k] int64, score [k], count): the eligible candidates by np.lexsort((idx, -score)), padded
    with -1 / -inf."""
    cand = np.flatnonzero(ok)
    order = cand[np.lexsort((cand, -scores_row[cand]))][:k]
    idx = np.full(k, -1, np.int64)
    score = np.full(k, -np.inf, np.float64)
    idx[:len(order)] = order
    score[:len(order)] = scores_row[order]
    return idx, score, len(order)


def topk(query_feat, cand_feat, queries, k, excl_ptr=None, excl_idx=None, cand_mask=None, scores=None):
    """(idx [n, k], score [n, k] fp64, count [n]) for every query; `scores` overrides the cosines."""
    s = cosines(query_feat, cand_feat, queries) if scores is None else scores
    out = [select(s[i], eligible(s[i], int(q), excl_ptr, excl_idx, cand_mask), k) for i, q in enumerate(queries)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32))


def check_tolerant(idx, score, count, s64_row, ok, k, tol):
    """One query's result against fp64 scores under an fp32 score error of `tol`: right count and
    padding, distinct eligible indices, scores within tol, nothing returned from below the k-th best
    by more than 2 tol, nothing above it by more than 2 tol left out, order non-increasing with
    ascending indices among equal scores."""
    n_ok = int(ok.sum())
    want = min(k, n_ok)
    assert count == want, (count, want)
    assert np.all(idx[want:] == -1) and np.all(np.isneginf(score[want:]))
    got = idx[:want]
    assert len(set(got.tolist())) == want and np.all(got >= 0) and np.all(ok[got])
    assert np.all(np.abs(score[:want].astype(np.float64) - s64_row[got]) <= tol)
    if want:
        t = np.sort(s64_row[ok])[::-1][want - 1]  # the k-th best fp64 score
        assert np.all(s64_row[got] >= t - 2 * tol)
        must = np.flatnonzero(ok & (s64_row > t + 2 * tol))
        assert np.isin(must, got).all()
    sc = score[:want]
    assert np.all(sc[:-1] >= sc[1:])
    same = sc[:-1] == sc[1:]
    assert np.all(got[:-1][same] < got[1:][same])
