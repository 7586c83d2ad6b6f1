"""Host-side index structures the GPU catalogue sampler reads (built once per dataset)."""
import numpy as np


def user_split_ranks(user_idx, item_idx, n_users, split_items):
    """CSR over users of the sorted, distinct ranks (positions in `split_items`) of each user's
    interacted items that belong to the split.

    This is the information datasets/dcuedataset.py:214-218 recomputes per sample with np.in1d over
    every item (`items = item_user.getcol(i).nonzero()[0]`; non-items = split songs minus items):
    the GPU sampler turns a draw r into the r-th non-item by skipping these ranks.
    """
    split_items = np.asarray(split_items, dtype=np.int64)
    user_idx = np.asarray(user_idx, dtype=np.int64)
    item_idx = np.asarray(item_idx, dtype=np.int64)
    n = len(split_items)
    pos = np.searchsorted(split_items, item_idx)
    inside = pos < n
    inside[inside] = split_items[pos[inside]] == item_idx[inside]
    key = np.unique(user_idx[inside] * (n + 1) + pos[inside])
    u, r = key // (n + 1), key % (n + 1)
    indptr = np.zeros(n_users + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(u, minlength=n_users)[:n_users])
    return indptr, r.astype(np.int32)


def saturated_users(indptr, n_split):
    """Users who interacted with every song of the split: the reference's
    np.random.choice(nonitems, N) raises ValueError for them (datasets/dcuedataset.py:219, an empty
    `nonitems`). The GPU sampler writes -1 for such a row; callers check batches against this set
    on the host first and raise as the reference does."""
    return np.nonzero(np.diff(np.asarray(indptr, dtype=np.int64)) >= int(n_split))[0]


MAX_TOTAL_WEIGHT = 2 ** 32 - 1  # every draw is one bounded 32-bit integer


def weighted_split_tables(indptr, ranks, weights):
    """The uint32 tables dcue_sample_catalogue_weighted reads (include/dcue.h dcue_weight_tables), from
    the user -> split-rank CSR and the integer weight of every split position:
      cum [n_split + 1]      exclusive prefix of the weights
      user_key [nnz]         K_e = cum[rank_e] - E_e
      user_skip [nnz]        E_e = the weights of the user's earlier entries
      user_weight [n_users]  W_u = sum(weights) - the weights of the user's entries
    ValueError for a negative weight, a rank outside the weights (or an indptr that does not cover
    `ranks`), and a total above 2^32 - 1."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    w = np.asarray(weights)
    if w.ndim != 1 or not (np.issubdtype(w.dtype, np.integer) or w.dtype == np.bool_):
        raise ValueError("weights must be a 1-d integer array")
    if len(w) and int(w.min()) < 0:
        raise ValueError("negative weight")
    inside = not len(ranks) or 0 <= int(ranks.min()) <= int(ranks.max()) < len(w)
    if len(indptr) < 1 or int(indptr[0]) != 0 or int(indptr[-1]) != len(ranks) or not inside:
        raise ValueError("length mismatch: the ranks index %d weights" % len(w))
    if len(w) and int(w.max()) > MAX_TOTAL_WEIGHT:
        raise ValueError("the weights sum past 2^32 - 1")
    w = w.astype(np.uint64)
    cum = np.zeros(len(w) + 1, dtype=np.uint64)
    np.cumsum(w, out=cum[1:])
    if int(cum[-1]) > MAX_TOTAL_WEIGHT:
        raise ValueError("the weights sum past 2^32 - 1 (%d)" % int(cum[-1]))
    run = np.zeros(len(ranks) + 1, dtype=np.uint64)  # prefix of w[rank] over the whole CSR
    np.cumsum(w[ranks], out=run[1:])
    first = run[indptr[:-1]]
    skip = run[:-1] - np.repeat(first, np.diff(indptr))
    key = cum[ranks] - skip
    user_weight = cum[-1] - (run[indptr[1:]] - first)
    return (cum.astype(np.uint32), key.astype(np.uint32), skip.astype(np.uint32), user_weight.astype(np.uint32))


def weighted_saturated_users(user_weight):
    """Users whose candidates' weights sum to zero (weighted_split_tables' user_weight): numpy's
    randint(0, 0) raises ValueError for them, the GPU sampler writes -1. check_catalogue_users takes
    this set as it takes saturated_users'."""
    return np.nonzero(np.asarray(user_weight) == 0)[0]


def popularity_weights(counts, alpha):
    """Integer weights in proportion to counts ** alpha, deterministic: f = counts ** alpha in float64;
    all f equal (alpha == 0 among them): ones, the uniform sampler's bits. Otherwise S is the largest
    power of two, at most 2^20, with sum(floor(f * S)) + n <= 2^32 - 1, and w = max(1, floor(f * S)):
    every song keeps a chance and the total fits 32 bits. f * S is exact (a power of two), so the
    weights depend on the counts alone. ValueError for alpha < 0 or a count below 1."""
    counts = np.asarray(counts)
    alpha = float(alpha)
    if not alpha >= 0.0 or not np.isfinite(alpha):
        raise ValueError("alpha must be a finite number >= 0, got %r" % (alpha,))
    if len(counts) and not (counts >= 1).all():
        raise ValueError("every song of the split needs a count >= 1")
    f = counts.astype(np.float64) ** alpha
    n = len(f)
    if n == 0 or (f == f[0]).all():
        return np.ones(n, dtype=np.uint32)
    if n >= MAX_TOTAL_WEIGHT or not np.isfinite(f).all():
        raise ValueError("the weights cannot fit a total of 2^32 - 1")
    scale = 2.0 ** 20
    while True:
        v = np.floor(f * scale)
        if float(v.max()) < 2.0 ** 32 and int(v.astype(np.uint64).sum()) + n <= MAX_TOTAL_WEIGHT:
            return np.maximum(v, 1.0).astype(np.uint32)
        scale *= 0.5  # ends: at a small enough scale every floor is 0 and n alone is within the bound


def check_catalogue_users(users, saturated):
    """Raise numpy's ValueError if a batch row's user has no candidate negative."""
    if len(saturated) and np.isin(np.asarray(users), saturated).any():
        raise ValueError("a cannot be empty unless no samples are taken")
