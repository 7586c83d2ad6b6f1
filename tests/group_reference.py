"""numpy / Python restatement of include/dcue.h's group-aware serving (dcue_list_group_cap,
dcue_list_group_stats, dcue_list_group_stats_mean), written as the definitions read: the cap is the
SEQUENTIAL greedy walk (keep an entry while its group holds fewer than `cap` kept ones), not the order-free
count the kernel uses, so agreement proves the two are the same rule.

Flags: BAD_INDEX = 2, SHORT = 8, BAD_GROUP = 16.
"""
import numpy as np

BAD_INDEX, SHORT, BAD_GROUP = 2, 8, 16
NEG_INF = np.float32(-np.inf)


def _clamp(x, hi):
    return max(0, min(int(x), hi))


def _entry_flags(entries, group_of, n_groups):
    """Flags of a sequence of candidate indices: out of [0, n_cand) / an in-range entry's bad group."""
    f = 0
    for v in entries:
        if v < 0 or v >= len(group_of):
            f |= BAD_INDEX
        elif group_of[v] < -1 or group_of[v] >= n_groups:
            f |= BAD_GROUP
    return f


def cap_one(idx, score, count, group_of, n_groups, cap, k_out, carry=None):
    """One list: (out_idx [k_out] int32, out_score [k_out] float32, out_count, dropped, flags)."""
    pool = len(idx)
    c = _clamp(count, pool)
    out_i, out_s = [], []
    if carry is not None:
        kc = _clamp(carry[2], k_out)
        out_i, out_s = [int(v) for v in carry[0][:kc]], [np.float32(s) for s in carry[1][:kc]]
    f = _entry_flags(out_i, group_of, n_groups) | _entry_flags([int(v) for v in idx[:c]], group_of, n_groups)
    oi, os_ = np.full(k_out, -1, np.int32), np.full(k_out, NEG_INF, np.float32)
    if f:
        return oi, os_, 0, 0, f
    held = {}  # group -> entries kept so far
    for v in out_i:
        g = int(group_of[v])
        if g >= 0:
            held[g] = held.get(g, 0) + 1
    dropped = 0
    for j in range(c):  # the sequential walk: it stops when the list is full
        if len(out_i) >= k_out:
            break
        v = int(idx[j])
        g = int(group_of[v])
        if g >= 0 and held.get(g, 0) >= cap:
            dropped += 1
            continue
        if g >= 0:
            held[g] = held.get(g, 0) + 1
        out_i.append(v)
        out_s.append(np.float32(score[j]))
    n = len(out_i)
    oi[:n], os_[:n] = out_i, out_s
    return oi, os_, n, dropped, SHORT if n < k_out else 0


def cap(idx, score, count, group_of, n_groups, cap_, k_out, carry=None):
    """All lists: (out_idx [n, k_out], out_score [n, k_out], out_count [n], dropped [n], flags [n])."""
    rows = [cap_one(idx[q], score[q], count[q], group_of, n_groups, cap_, k_out,
                    None if carry is None else (carry[0][q], carry[1][q], carry[2][q])) for q in range(len(idx))]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32),
            np.array([r[4] for r in rows], np.int32))


def cap_full_ranking(ranking, scores, group_of, cap_, k):
    """The cap applied to a FULL ranking (every eligible candidate, best first): the first k survivors --
    what deepening must reach. (idx list, score list)."""
    held, oi, os_ = {}, [], []
    for v, s in zip(ranking, scores):
        g = int(group_of[v])
        if len(oi) >= k:
            break
        if g >= 0 and held.get(g, 0) >= cap_:
            continue
        if g >= 0:
            held[g] = held.get(g, 0) + 1
        oi.append(int(v))
        os_.append(np.float32(s))
    return oi, np.array(os_, np.float32)


def stats(idx, count, group_of, n_groups, ks, exposure=None):
    """(stats int32 [n, m, 2] = (distinct, top), flags [n]); exposure int64 [m, n_groups] is added to."""
    n, k = idx.shape
    out = np.zeros((n, len(ks), 2), np.int32)
    flags = np.zeros(n, np.int32)
    for q in range(n):
        c = _clamp(count[q], k)
        L = [int(v) for v in idx[q, :c]]
        flags[q] = _entry_flags(L, group_of, n_groups)
        if flags[q]:
            continue
        G = [int(group_of[v]) for v in L]
        for i, K in enumerate(ks):
            head = G[:min(K, c)]
            sizes = {}
            for g in head:
                if g >= 0:
                    sizes[g] = sizes.get(g, 0) + 1
            loose = sum(1 for g in head if g < 0)
            out[q, i, 0] = len(sizes) + loose
            out[q, i, 1] = max(list(sizes.values()) + ([1] if loose else [0]))
        if exposure is not None:
            for j, g in enumerate(G):
                slot = next((i for i, K in enumerate(ks) if j < K), None)
                if g >= 0 and slot is not None:
                    exposure[slot, g] += 1
    return out, flags


def stats_mean(st, flags, exposure=None, present=None):
    """(mean float64 [m, 2], coverage float64 [m] or None, n_evaluated): one division of an exact integer
    sum per value."""
    keep = flags == 0
    n = int(keep.sum())
    tot = st[keep].astype(np.int64).sum(axis=0)
    mean = tot.astype(np.float64) / np.float64(n) if n else np.zeros(tot.shape, np.float64)
    cov = None
    if exposure is not None:
        seen = np.cumsum(exposure != 0, axis=0) > 0  # exposed in cutoffs 0..i
        den = int((present != 0).sum()) if present is not None else exposure.shape[1]
        cov = seen.sum(axis=1).astype(np.float64) / np.float64(den) if den else np.zeros(len(exposure))
    return mean, cov, n
