"""Weighted catalogue negatives, the definition in plain numpy (no dependency on the library).

For one sample of user u over the sorted split items, integer weights w by split position and the
user's sorted split ranks rho_u:

    cand = positions 0..n-1 not in rho_u              (ascending)
    cw   = cumsum(w[cand]);  W_u = cw[-1]
    r    = randint(0, W_u, N)                         (legacy RandomState)
    neg  = split_items[cand[searchsorted(cw, r, side='right')]]

W_u == 0: numpy raises ValueError; the row is -1 and no draw is consumed (what the GPU sampler writes;
callers raise on the host first). W_u == 1: randint(0, 1, N) consumes nothing.
"""
import numpy as np


def sample(rs, split_items, weights, ranks, N):
    """One sample from the stream `rs` (a RandomState, or the np.random module for the global one)."""
    split_items = np.asarray(split_items, dtype=np.int64)
    w = np.asarray(weights).astype(np.int64)
    keep = np.ones(len(split_items), dtype=bool)
    keep[np.asarray(ranks, dtype=np.int64)] = False
    cand = np.nonzero(keep)[0]
    cw = np.cumsum(w[cand])
    total = int(cw[-1]) if len(cw) else 0
    if total == 0:
        return np.full(N, -1, dtype=np.int64)
    r = rs.randint(0, total, N)
    return split_items[cand[np.searchsorted(cw, r, side='right')]]


def sample_users(seed, reseed, split_items, weights, indptr, ranks, users, N):
    """[len(users)][N] item ids: all samples in order on RandomState(seed)'s stream, or (reseed) each
    after np.random.seed(seed) on the global stream, as DCUEDataset's random_seed mode."""
    rs = np.random.RandomState(seed)
    out = np.empty((len(users), N), dtype=np.int64)
    for i, u in enumerate(users):
        if reseed:
            np.random.seed(seed)
        out[i] = sample(np.random if reseed else rs, split_items, weights, ranks[indptr[u]:indptr[u + 1]], N)
    return out
