"""numpy fp64 reference of dcue_list_explain (include/dcue.h): for every pick of a list, the usable songs
of the query row's history by cosine descending, then candidate index ascending -- topk_reference's
cosines and order -- with the flags, and the tolerant comparison the GPU tests use where fp32
similarities may order near-ties differently."""
import numpy as np

import topk_reference as T

MAX_REASONS = 8
FLAG_NO_HISTORY, FLAG_BAD_INDEX, FLAG_NONFINITE = 1, 2, 4


def history(u, hist_ptr, hist_idx, n_cand, hist_mask=None):
    """(H_u int64 ascending, bad): the row's entries whose mask byte is non-zero; bad: an entry lies
    outside [0, n_cand) (each is range-checked before it addresses the mask)."""
    row = np.asarray(hist_idx[hist_ptr[u]:hist_ptr[u + 1]], np.int64)
    if np.any((row < 0) | (row >= n_cand)):
        return np.zeros(0, np.int64), True
    if hist_mask is not None:
        row = row[np.asarray(hist_mask)[row] != 0]
    return row, False


def explain_list(lst, count, u, hist_ptr, hist_idx, feat, m, hist_mask=None, n_query_rows=None):
    """(why_idx [k, m] int64, why_sim [k, m] fp64, flags) of one list."""
    lst = np.asarray(lst, np.int64)
    k, n_cand = len(lst), len(feat)
    n_rows = len(hist_ptr) - 1 if n_query_rows is None else n_query_rows
    c = min(max(int(count), 0), k)
    why_idx = np.full((k, m), -1, np.int64)
    why_sim = np.full((k, m), -np.inf, np.float64)
    if not 0 <= u < n_rows or np.any((lst[:c] < 0) | (lst[:c] >= n_cand)):
        return why_idx, why_sim, FLAG_BAD_INDEX
    H, bad = history(u, hist_ptr, hist_idx, n_cand, hist_mask)
    if bad:
        return why_idx, why_sim, FLAG_BAD_INDEX
    if len(H) == 0:
        return why_idx, why_sim, FLAG_NO_HISTORY
    flags = 0
    if c:
        s = T.cosines(feat, feat[H], lst[:c])  # [c][|H|]
        if not np.all(np.isfinite(s)):
            flags |= FLAG_NONFINITE
        for j in range(c):
            idx, sim, n = T.select(s[j], ~np.isnan(s[j]), m)
            why_idx[j, :n], why_sim[j, :n] = H[idx[:n]], sim[:n]
    return why_idx, why_sim, flags


def explain(lists, counts, queries, hist_ptr, hist_idx, feat, m, hist_mask=None, n_query_rows=None):
    """(why_idx [n, k, m], why_sim [n, k, m], flags [n]) of every list."""
    out = [explain_list(lists[q], counts[q], int(queries[q]), hist_ptr, hist_idx, feat, m, hist_mask, n_query_rows)
           for q in range(len(lists))]
    k = np.asarray(lists).shape[1]
    if not out:
        return np.zeros((0, k, m), np.int64), np.zeros((0, k, m)), np.zeros(0, np.int32)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32)


def explain_brute(lst, count, u, hist_ptr, hist_idx, feat, m, hist_mask=None):
    """The same for valid inputs, restated pair by pair: [(index, similarity), ...] per position j < c."""
    f = np.asarray(feat, np.float64)
    out = []
    for a in list(lst)[:min(max(int(count), 0), len(lst))]:
        pairs = []
        for h in hist_idx[hist_ptr[u]:hist_ptr[u + 1]]:
            if hist_mask is not None and not hist_mask[h]:
                continue
            xa = f[a] / max(np.sqrt(np.dot(f[a], f[a])), 1e-8)
            xh = f[h] / max(np.sqrt(np.dot(f[h], f[h])), 1e-8)
            s = float(np.dot(xa, xh))
            if s == s:
                pairs.append((int(h), s))
        pairs.sort(key=lambda p: (-p[1], p[0]))
        out.append(pairs[:m])
    return out


def check_tolerant(why_idx, why_sim, lst, count, u, hist_ptr, hist_idx, feat, m, tol, hist_mask=None):
    """One list's GPU result against fp64 under an fp32 similarity error of `tol`: per position j < c
    topk_reference.check_tolerant over the usable history (right count and padding, similarities within
    tol, near-ties within 2 tol of the m-th best either way, nothing else); rows j >= c all padding."""
    k, n_cand = len(lst), len(feat)
    c = min(max(int(count), 0), k)
    H, bad = history(u, hist_ptr, hist_idx, n_cand, hist_mask)
    assert not bad
    ok = np.zeros(n_cand, bool)
    ok[H] = True
    s64 = T.cosines(feat, feat, np.asarray(lst[:c], np.int64)) if c else np.zeros((0, n_cand))
    for j in range(c):
        n = int((why_idx[j] >= 0).sum())
        T.check_tolerant(np.asarray(why_idx[j], np.int64), why_sim[j], n, s64[j], ok & ~np.isnan(s64[j]), m, tol)
    assert np.all(why_idx[c:] == -1) and np.all(np.isneginf(why_sim[c:]))
