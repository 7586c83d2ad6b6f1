"""The definition of dcue_select_negatives (include/dcue.h) in numpy, with fp64 scores.

select(user_feat, item_feat, users, pool, N, H) -> (out [n, N] int64, hard [n] int32, flags [n] int32).
check_against(...) is the tolerance check the GPU tests hold every row to: fp32 scores may order two
candidates the other way round only where their fp64 scores are closer than tau."""
import numpy as np

FLAG_NONFINITE, FLAG_BAD_ID = 1, 2
EPS = 1e-8


def cosines(u, rows):
    """nn.CosineSimilarity's value of u against each of rows, in fp64: u.c / (max(|u|, eps) max(|c|, eps))."""
    u = np.asarray(u, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(u))
    with np.errstate(all="ignore"):
        un = np.maximum(np.sqrt(np.sum(u * u)), EPS)
        cn = np.maximum(np.sqrt(np.sum(rows * rows, axis=1)), EPS)
        return np.sum(rows * u, axis=1) / (un * cn)  # a NaN anywhere in either row gives NaN


def row_scores(user_feat, item_feat, user, ids):
    """(scores fp64 [P] (0 where there is no score), in_range bool [P], eligible bool [P]) of one row."""
    ids = np.asarray(ids, dtype=np.int64)
    n_items = len(item_feat)
    in_range = (ids >= 0) & (ids < n_items)
    s = np.zeros(len(ids), dtype=np.float64)
    if in_range.any():
        s[in_range] = cosines(user_feat[user], item_feat[ids[in_range]])
    first = np.zeros(len(ids), dtype=bool)
    first[np.unique(ids, return_index=True)[1]] = True
    return s, in_range, in_range & first & ~np.isnan(s)


def fill(ids, hard_pos, N):
    """The row given its hard positions: their ids in ascending position, then the leading others."""
    hard_pos = np.sort(np.asarray(hard_pos, dtype=np.int64))
    rest = np.setdiff1d(np.arange(len(ids)), hard_pos)[:N - len(hard_pos)]
    return np.concatenate([np.asarray(ids, dtype=np.int64)[hard_pos], np.asarray(ids, dtype=np.int64)[rest]])


def score_table(user_feat, item_feat, users, pool):
    """row_scores of every row with a user inside the table (None for the others): computed once and
    shared by select() / check_against() calls over the same rows (table=)."""
    return [row_scores(user_feat, item_feat, u, ids) if 0 <= u < len(user_feat) else None
            for u, ids in zip(np.asarray(users, dtype=np.int64), np.asarray(pool, dtype=np.int64))]


def select(user_feat, item_feat, users, pool, N, H, table=None):
    pool = np.asarray(pool, dtype=np.int64)
    users = np.asarray(users, dtype=np.int64)
    n, P = pool.shape
    assert 1 <= N <= P and 0 <= H <= N
    out = np.zeros((n, N), dtype=np.int64)
    hard = np.zeros(n, dtype=np.int32)
    flags = np.zeros(n, dtype=np.int32)
    for b in range(n):
        if not 0 <= users[b] < len(user_feat):
            flags[b] = FLAG_BAD_ID
            out[b] = pool[b, :N]
            continue
        s, in_range, elig = row_scores(user_feat, item_feat, users[b], pool[b]) if table is None else table[b]
        if not in_range.all():
            flags[b] |= FLAG_BAD_ID
        if not np.isfinite(s[in_range]).all():
            flags[b] |= FLAG_NONFINITE
        pos = np.flatnonzero(elig)
        order = pos[np.argsort(-s[pos], kind="stable")]  # score descending, position ascending
        chosen = order[:H]
        hard[b] = len(chosen)
        out[b] = fill(pool[b], chosen, N)
    return out, hard, flags


def tau(d):
    """Three fp32 sums of at most max(d, 32) terms, two scores compared, 2^-24 relative rounding each."""
    return 4 * max(d, 32) * 2.0 ** -24


def check_against(user_feat, item_feat, users, pool, N, H, out, hard, tol=None, table=None):
    """Assert, for every row, that (out, hard) is a selection the definition allows within tol (default
    tau(d)): h exact, the hard positions ascending, eligible and no worse than the h-th best fp64 score
    by more than tol, no unchosen eligible position better than it by more than tol, and the fill exactly
    the definition's given those hard positions. Returns the number of rows equal to select()'s."""
    pool = np.asarray(pool, dtype=np.int64)
    out = np.asarray(out)
    tol = tau(user_feat.shape[1]) if tol is None else tol
    want_out, want_hard, _ = select(user_feat, item_feat, users, pool, N, H, table)
    assert np.array_equal(np.asarray(hard), want_hard), "out_hard differs"
    same = 0
    for b in range(len(pool)):
        h = int(want_hard[b])
        if np.array_equal(out[b], want_out[b]):
            same += 1
            continue
        assert h > 0, "row %d: no hard negative, yet not the plain draws" % b
        s, _, elig = row_scores(user_feat, item_feat, users[b], pool[b]) if table is None else table[b]
        F = np.flatnonzero(elig)
        # the hard ids are distinct first occurrences: each names its position
        first_pos = {int(pool[b, p]): int(p) for p in F}
        assert all(int(i) in first_pos for i in out[b, :h]), "row %d: a hard id is not eligible" % b
        hp = np.array([first_pos[int(i)] for i in out[b, :h]], dtype=np.int64)
        assert (np.diff(hp) > 0).all(), "row %d: hard positions not ascending" % b
        t = np.sort(s[F])[::-1][h - 1]
        assert (s[hp] >= t - tol).all(), "row %d: a hard score is below the boundary by %.3e" % (b, float((t - s[hp]).max()))
        rest = np.setdiff1d(F, hp)
        assert (s[rest] <= t + tol).all(), "row %d: an unchosen score is above the boundary by %.3e" % (b, float((s[rest] - t).max()))
        assert np.array_equal(out[b], fill(pool[b], hp, N)), "row %d: the fill is not the definition's" % b
    return same
