"""numpy reference of include/dcue.h's dcue_list_mmr / dcue_list_ild / dcue_list_ild_mean: the header's
definitions implemented literally in fp64 (dtype=np.float32: the same steps in fp32, an emulation of the
kernel's arithmetic up to its summation order), and the tolerant check the GPU tests apply where fp32
rounding may legitimately change a pick."""
import numpy as np

REL_RAW, REL_MINMAX = 0, 1
FLAG_NO_PAIR, FLAG_BAD_INDEX, FLAG_NONFINITE = 1, 2, 4
EPS = 1e-8  # the project's norm clamp


def tol_sim(d):
    """Bound on |fp32 similarity - exact similarity|: (2 dp + 16) 2^-24, dp = d rounded up to 16. The
    fp32 dot's error is <= d 2^-24 ||x|| ||y|| (Cauchy-Schwarz); the two fp32 norms (read from the Gram
    diagonal, so each carries the same bound) and the two scalings add the rest -- the project's cosine
    tolerance (dp + 8) 2^-24 doubled."""
    dp = (d + 15) // 16 * 16
    return (2 * dp + 16) * 2.0 ** -24


def tol_rel(rel_mode):
    """0 for raw relevance (used as is); 4 2^-24 for min-max: two subtractions and a division in fp32 of
    a value in [0, 1]."""
    return 0.0 if rel_mode == REL_RAW else 4 * 2.0 ** -24


def sims(cand_feat, lst, dtype=np.float64):
    """[c, c] cosine of rows lst of cand_feat with the clamp x / max(||x||, 1e-8) on each side."""
    X = np.asarray(cand_feat)[np.asarray(lst, dtype=np.int64)].astype(dtype)
    if dtype == np.float64:
        n = np.maximum(np.sqrt((X * X).sum(axis=1)), EPS)
        Xn = X / n[:, None]
        return Xn @ Xn.T
    G = (X @ X.T).astype(np.float32)  # the kernel's route: Gram, norms from its diagonal
    inv = (np.float32(1) / np.maximum(np.sqrt(np.diag(G)), np.float32(EPS))).astype(np.float32)
    return (G * (inv[:, None] * inv[None, :]).astype(np.float32)).astype(np.float32)


def scale_rel(rel, rel_mode, dtype=np.float64):
    r = np.asarray(rel, dtype=np.float32).astype(dtype)
    if rel_mode == REL_RAW or len(r) == 0:
        return r
    lo, hi = r.min(), r.max()
    return np.zeros_like(r) if hi == lo else ((r - lo) / (hi - lo)).astype(dtype)


def values(rp, m, lam, first, dtype=np.float64):
    """f_a = lam r'_a - (1 - lam) m_a (m_a = 0 while nothing is selected), every operation in dtype."""
    lam = dtype(lam)
    mm = np.zeros_like(m) if first else m
    return ((lam * rp).astype(dtype) - ((dtype(1) - lam) * mm).astype(dtype)).astype(dtype) + dtype(0)


def list_flags(lst, rel, c, cand_feat):
    lst = np.asarray(lst)[:c]
    if np.any((lst < 0) | (lst >= len(cand_feat))):
        return FLAG_BAD_INDEX
    ok = np.isfinite(np.asarray(cand_feat)[lst]).all() and (rel is None or np.isfinite(np.asarray(rel)[:c]).all())
    return 0 if ok else FLAG_NONFINITE


def mmr(lst, rel, c, cand_feat, k_out, lam, rel_mode, dtype=np.float64):
    """(idx int32 [k_out], score float32 [k_out], count, flags) of one list: greedy MMR, ties to the
    lowest pool position; short lists padded with -1 / -inf; a flagged list comes back empty."""
    c = int(min(max(c, 0), len(lst)))
    out_idx = np.full(k_out, -1, np.int32)
    out_score = np.full(k_out, -np.inf, np.float32)
    flags = list_flags(lst, rel, c, cand_feat)
    if flags or c == 0:
        return out_idx, out_score, 0, flags
    lst, rel = np.asarray(lst)[:c], np.asarray(rel, dtype=np.float32)[:c]
    S = sims(cand_feat, lst, dtype)
    rp = scale_rel(rel, rel_mode, dtype)
    m = np.zeros(c, dtype)
    open_ = np.ones(c, bool)
    n_sel = min(k_out, c)
    for t in range(n_sel):
        f = values(rp, m, lam, t == 0, dtype)
        a = int(np.argmax(np.where(open_, f, -np.inf)))  # the first maximum: the lowest position
        if not open_[a]:  # (every open f is -inf)
            a = int(np.argmax(open_))
        open_[a] = False
        out_idx[t], out_score[t] = lst[a], rel[a]
        m = S[a].copy() if t == 0 else np.maximum(m, S[a])
    return out_idx, out_score, n_sel, 0


def mmr_brute(lst, rel, c, cand_feat, k_out, lam, rel_mode):
    """The same selection restated without running state: at each step every candidate's redundancy is
    recomputed from the selected set (positions returned, not indices)."""
    S = sims(cand_feat, np.asarray(lst)[:c])
    rp = scale_rel(np.asarray(rel)[:c], rel_mode)
    picked = []
    for _ in range(min(k_out, c)):
        best, best_f = None, None
        for a in range(c):
            if a in picked:
                continue
            red = max((S[a, b] for b in picked), default=0.0)
            f = lam * rp[a] - (1 - lam) * red
            if best is None or f > best_f:
                best, best_f = a, f
        picked.append(best)
    return picked


def ild(lst, c, cand_feat, ks):
    """(values float64 [m], flags) of one list at the ascending cutoffs ks."""
    c = int(min(max(c, 0), len(lst)))
    out = np.zeros(len(ks), np.float64)
    flags = list_flags(lst, None, c, cand_feat)
    if flags:
        return out, flags
    S = sims(cand_feat, np.asarray(lst)[:c]) if c else np.zeros((0, 0))
    for i, K in enumerate(ks):
        n = min(K, c)
        if n < 2:
            flags |= FLAG_NO_PAIR
            continue
        iu = np.triu_indices(n, 1)
        out[i] = 2.0 / (n * (n - 1)) * (1.0 - S[:n, :n][iu]).sum()
    return out, flags


def ild_means(values_, flags):
    """(mean [m], n) over the unflagged rows."""
    keep = np.asarray(flags) == 0
    n = int(keep.sum())
    v = np.asarray(values_, np.float64)
    return (v[keep].sum(axis=0) / n if n else np.zeros(v.shape[1])), n


def check_greedy_tolerant(got_idx, got_score, got_count, lst, rel, c, cand_feat, k_out, lam, rel_mode):
    """Checks one list's GPU (or fp32-emulated) output against the fp64 definitions where rounding may
    change a pick: count, padding, distinct pool positions, out_score = the entry's relevance bit for
    bit, and at every step t -- with the output's own first t picks as S -- that the picked entry's fp64
    f is within 2 ((1 - lam) tol_sim + lam tol_rel) of the best remaining one. Returns (steps, steps
    whose pick is not the fp64 strict argmax under that prefix)."""
    c = int(min(max(c, 0), len(lst)))
    lst, rel = np.asarray(lst)[:c], np.asarray(rel, dtype=np.float32)[:c]
    n_sel = min(k_out, c)
    assert int(got_count) == n_sel, (got_count, n_sel)
    assert np.all(np.asarray(got_idx)[n_sel:] == -1) and np.all(np.asarray(got_score)[n_sel:] == -np.inf)
    d = np.asarray(cand_feat).shape[1]
    slack = 2 * ((1 - lam) * tol_sim(d) + lam * tol_rel(rel_mode))
    S = sims(cand_feat, lst)
    rp = scale_rel(rel, rel_mode)
    open_ = np.ones(c, bool)
    m = np.zeros(c)
    differ = 0
    for t in range(n_sel):
        # the output's entry -> its pool position: the lowest open one with that index and relevance
        bits = np.float32(got_score[t]).view(np.uint32)
        match = np.flatnonzero(open_ & (lst == got_idx[t]) & (rel.view(np.uint32) == bits))
        assert len(match), "step %d: (%d, %r) is not an open pool entry" % (t, got_idx[t], got_score[t])
        a = int(match[0])
        f = np.where(open_, values(rp, m, lam, t == 0), -np.inf)
        assert f[a] >= f.max() - slack, "step %d: f = %.9g, best %.9g, slack %.3g" % (t, f[a], f.max(), slack)
        differ += a != int(np.argmax(f))
        open_[a] = False
        m = S[a].copy() if t == 0 else np.maximum(m, S[a])
    return n_sel, differ
