"""GPU tests of popularity-aware serving: dcue_topk_prior (rank.TopK prior=), dcue_list_item_stats /
dcue_exposure_gini (rank.PopStats), DCUE's popularity= / item_prior= / evaluate_topk(novelty=True) and the
train_dcue.py flags, against the restatements in popularity_reference.py.

The exact cases take every pair's plain score s0 from the library itself (dcue_topk_scored under masks that
admit 128 candidates at a time: score bits do not depend on the mask), so the prior call is held to
fl32(s0 + p) with == on indices, score bits and counts. Lattice cases (topk's: cosines on multiples of 1/16)
with priors on multiples of 2^-10 make every sum exact, and are held to the fp64 reference. Gaussian cases
are held to test_gpu_topk.py's bound for the same d plus one rounding of the sum, 2^-24 (1 + max|p|).
"""
import ctypes
import functools
import json

import numpy as np
import pandas as pd
import pytest
import torch

import popularity_reference as P
import topk_reference as T
from test_gpu_topk import _case as topk_case
from test_gpu_topk import _datasets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ROWS = 20


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------- the library call
def _call(c, k, score="cosine", prior=None, qb=None, split=0, excl=True, mask=True, scored=False):
    """dcue_topk_prior (scored: dcue_topk_scored, which takes no prior) as (idx, score, count, flags) numpy."""
    from dcrecommend import _native as nat
    qf, cand, q = _dev(c["qf"]), _dev(c["cand"]), _dev(np.asarray(c["queries"], np.int32))
    ptr, idx = (_dev(c["ptr"]), _dev(c["idx"] if len(c["idx"]) else np.zeros(1, np.int32))) if excl else (None, None)
    m = _dev(c["mask"] if mask is True else mask) if mask is not False else None
    p = _dev(np.asarray(prior, np.float32)) if prior is not None else None
    nq, n_cand, d = len(c["queries"]), len(c["cand"]), c["cand"].shape[1]
    qb = nq if qb is None else qb
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib().dcue_topk_workspace_bytes(n_cand, d, qb, k, split, ctypes.byref(nbytes)), "ws")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    out = (torch.full((nq, k), -7, dtype=torch.int32, device=DEV), torch.full((nq, k), 7.0, device=DEV),
           torch.full((nq,), -7, dtype=torch.int32, device=DEV), torch.full((nq,), -7, dtype=torch.int32, device=DEV))
    head = (nat.SCORES[score], nat.ptr(qf), len(c["qf"]), nat.ptr(cand), n_cand, d, nat.ptr(q), nq, nat.ptr(ptr),
            nat.ptr(idx), nat.ptr(m))
    tail = (k, qb, split, nat.ptr(ws), ws.numel(), *[nat.ptr(t) for t in out], nat.stream_handle(torch.device(DEV)))
    if scored:
        nat.check(nat.lib().dcue_topk_scored(*head, *tail), "dcue_topk_scored")
    else:
        nat.check(nat.lib().dcue_topk_prior(*head, nat.ptr(p), *tail), "dcue_topk_prior")
    return tuple(t.cpu().numpy() for t in out)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _s0(c, score):
    """float32 [n_queries, n_cand]: every pair's plain score, from the library itself."""
    n_cand, nq = len(c["cand"]), len(c["queries"])
    s0 = np.full((nq, n_cand), np.nan, np.float32)
    for lo in range(0, n_cand, 128):
        m = np.zeros(n_cand, np.uint8)
        m[lo:lo + 128] = 1
        idx, sc, count, flags = _call(c, 128, score, excl=False, mask=m, scored=True)
        n = min(128, n_cand - lo)
        assert (count == n).all() and not flags.any()
        for i in range(nq):
            s0[i, idx[i, :n]] = sc[i, :n]
    assert not np.isnan(s0).any()
    return s0


@functools.lru_cache(maxsize=None)
def _mk(seed, d, n_cand, nq, variant="dups"):
    """Gaussian factors with duplicated candidate rows -- half of the pairs with equal priors (a tie: the
    lower index first), half with different ones -- random exclusion rows, a random mask, a random prior.
    variant: "edges" (every row excludes the tile-edge candidates), "single" (a mask with a single one),
    "reverse" (set by the test: needs s0)."""
    rs = np.random.RandomState(seed)
    cand = rs.randn(n_cand, d).astype(np.float32)
    qf = rs.randn(N_ROWS, d).astype(np.float32)
    prior = (0.5 * rs.randn(n_cand)).astype(np.float32)
    n_dup = n_cand // 10
    if n_dup:
        src = rs.choice(n_cand, n_dup, replace=False)
        dst = rs.choice(n_cand, n_dup, replace=False)
        cand[dst] = cand[src]
        prior[dst[::2]] = prior[src[::2]]
    rows = []
    for r in range(N_ROWS):
        row = rs.choice(n_cand, rs.randint(0, min(10, n_cand - 1) + 1), replace=False)
        if variant == "edges":
            row = np.concatenate([row, [e for e in (63, 64, n_cand - 1) if e < n_cand]])
        if variant == "single":
            row = row[row != n_cand // 2]
        rows.append(np.unique(row))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)
    mask = (rs.rand(n_cand) < 0.8).astype(np.uint8)
    if variant == "single":
        mask[:] = 0
        mask[n_cand // 2] = 1
    return dict(qf=qf, cand=cand, ptr=ptr, idx=idx, mask=mask, queries=rs.randint(0, N_ROWS, nq), prior=prior)


# (d, n_cand, n_queries, k, cand_split): every d / n_cand / n_queries / k / cand_split the kernel branches on --
# the MT = 4 instances (d = 1, 100, 128), the QT = 32 / MT = 2 one (d = 256, k = 128), one candidate, a
# partial last tile, more than one split, one query, a ragged last query tile, more than one query tile
SHAPES = [(1, 1, 1, 1, 0), (1, 1000, 17, 1, 3), (100, 63, 17, 100, 1), (128, 65, 70, 128, 3), (128, 200, 1, 100, 0),
          (100, 1000, 70, 100, 3), (128, 1000, 70, 100, 0), (256, 1000, 70, 128, 3), (256, 200, 17, 128, 1)]


# ------------------------------------------------------------------------------- 1. null and zero prior
@pytest.mark.parametrize("score", ["cosine", "dot"])
@pytest.mark.parametrize("d,n_cand,nq,k,split", SHAPES)
def test_null_and_zero_prior_are_the_plain_call(d, n_cand, nq, k, split, score):
    c = _mk(11 + d + n_cand, d, n_cand, nq)
    plain = _call(c, k, score, split=split, scored=True)
    _same(_call(c, k, score, prior=None, split=split), plain)
    _same(_call(c, k, score, prior=np.zeros(n_cand, np.float32), split=split), plain)
    _same(_call(c, k, score, prior=-np.zeros(n_cand, np.float32), split=split), plain)


# ------------------------------------------------------------------------------- 2. the exact contract
def _assert_contract(c, k, score, split, prior, s0, excl=True, mask=True):
    got = _call(c, k, score, prior=prior, split=split, excl=excl, mask=mask)
    want = P.topk_prior(s0, prior, c["queries"], k, c["ptr"] if excl else None, c["idx"] if excl else None,
                        c["mask"] if mask else None)
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1]))
    assert not got[3].any() and not want[3].any()
    return got


@pytest.mark.parametrize("score", ["cosine", "dot"])
@pytest.mark.parametrize("d,n_cand,nq,k,split", SHAPES)
def test_prior_call_equals_the_restatement_on_the_librarys_scores(d, n_cand, nq, k, split, score):
    c = _mk(11 + d + n_cand, d, n_cand, nq)
    s0 = _s0(c, score)
    got = _assert_contract(c, k, score, split, c["prior"], s0)
    if n_cand in (63, 65):  # fewer eligible candidates than k: padded
        assert (got[2] < k).all() and (got[0][:, -1] == -1).all() and np.isneginf(got[1][:, -1]).all()
    _assert_contract(c, k, score, split, c["prior"], s0, excl=False, mask=False)


@pytest.mark.parametrize("d,n_cand,nq,k,split,variant", [(128, 200, 17, 128, 3, "edges"), (100, 1000, 70, 100, 3, "edges"),
                                                         (128, 200, 17, 100, 0, "single"), (256, 1000, 70, 128, 1, "single")])
def test_prior_call_with_edge_exclusions_and_a_single_one_mask(d, n_cand, nq, k, split, variant):
    c = _mk(5, d, n_cand, nq, variant)
    s0 = _s0(c, "cosine")
    got = _assert_contract(c, k, "cosine", split, c["prior"], s0)
    if variant == "edges":
        assert not np.isin(got[0], [63, 64, n_cand - 1]).any()
    else:
        assert (got[2] == 1).all() and (got[0][:, 0] == n_cand // 2).all()


@pytest.mark.parametrize("d,n_cand,k,split", [(128, 200, 128, 0), (100, 1000, 100, 3), (256, 1000, 128, 3)])
def test_a_prior_that_reverses_the_whole_order(d, n_cand, k, split):
    """One query, prior = -2 s0 (exact): every sum is -s0, so the list is the plain ranking's far end."""
    c = _mk(9, d, n_cand, 1)
    s0 = _s0(c, "cosine")
    prior = (np.float32(-2.0) * s0[0]).astype(np.float32)
    assert np.array_equal(_bits(P.prior_scores(s0, prior)), _bits(-s0 + np.float32(0.0)))
    got = _assert_contract(c, k, "cosine", split, prior, s0, excl=False, mask=False)
    worst = np.lexsort((np.arange(n_cand), s0[0]))[:k]  # ascending plain score, ties by ascending index
    assert got[0][0].tolist() == worst.tolist()


# ------------------------------------------------------------------------------- 3. lattice
@pytest.mark.parametrize("d,k", [(100, 100), (128, 128), (256, 128)])
def test_lattice_with_dyadic_priors_equals_fp64(d, k):
    from dcrecommend.nn import rank
    c = topk_case(5 + d, 130, 2500, d, 150, True)
    rs = np.random.RandomState(d)
    prior = (rs.randint(-1024, 1025, len(c["cand"])) / 1024.0).astype(np.float32)  # multiples of 2^-10 in [-1, 1]
    prior[::7] = prior[3]  # equal priors on unequal and equal rows: ties stay ties
    tk = rank.TopK(c["ptr"], c["idx"], c["mask"], DEV)
    idx, score, count = tk.topk(_dev(c["qf"]), _dev(c["cand"]), c["queries"], k, prior=prior)
    want = T.topk(None, None, c["queries"], k, c["ptr"], c["idx"], c["mask"], scores=c["s64"] + prior.astype(np.float64))
    assert np.array_equal(count, want[2]) and np.array_equal(idx, want[0])
    assert np.array_equal(_bits(score), _bits(want[1] + 0.0))


# ------------------------------------------------------------------------------- 4. Gaussian against fp64
@pytest.mark.parametrize("d", [100, 128])
def test_gaussian_with_prior_vs_fp64(d):
    from dcrecommend.nn import rank
    k = 50
    c = topk_case(70 + d, 130, 5003, d, 130, False)
    prior = (0.3 * np.random.RandomState(d).randn(len(c["cand"]))).astype(np.float32)
    tk = rank.TopK(c["ptr"], c["idx"], c["mask"], DEV)
    idx, score, count = tk.topk(_dev(c["qf"]), _dev(c["cand"]), c["queries"], k, prior=prior)
    # test_gpu_topk's bound for this d, plus one rounding of the sum (|s0 + p| <= 1 + max|p|)
    tol = ((d + 15) // 16 * 16 + 8) * 2.0 ** -24 + 2.0 ** -24 * (1.0 + float(np.abs(prior).max()))
    s64 = c["s64"] + prior.astype(np.float64)
    for i, q in enumerate(c["queries"]):
        ok = T.eligible(s64[i], int(q), c["ptr"], c["idx"], c["mask"])
        T.check_tolerant(idx[i], score[i], int(count[i]), s64[i], ok, k, tol)


# ------------------------------------------------------------------------------- 5. invariance
@pytest.mark.parametrize("d,n_cand,nq,k", [(128, 1000, 70, 100), (256, 1000, 17, 128), (1, 200, 70, 1)])
@pytest.mark.parametrize("score", ["cosine", "dot"])
def test_lists_do_not_depend_on_query_batch_or_cand_split(d, n_cand, nq, k, score):
    c = _mk(21, d, n_cand, nq)
    first = _call(c, k, score, prior=c["prior"], qb=nq, split=1)
    _same(_call(c, k, score, prior=c["prior"], qb=1, split=1), first)
    _same(_call(c, k, score, prior=c["prior"], qb=nq, split=3), first)
    _same(_call(c, k, score, prior=c["prior"], qb=16, split=0), first)


# ------------------------------------------------------------------------------- 6. non-finite
@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("d,n_cand,nq,k,split", [(128, 1000, 70, 100, 3), (256, 200, 17, 128, 0)])
def test_nonfinite_prior_flags_the_queries_that_could_see_it(d, n_cand, nq, k, split, value):
    from dcrecommend.nn import rank
    c = dict(_mk(31, d, n_cand, nq))
    first = next(int(q) for q in c["queries"] if c["ptr"][q + 1] > c["ptr"][q])
    seen = int(c["idx"][c["ptr"][first]])  # a candidate one query's row excludes (and few others do)
    c["mask"] = c["mask"].copy()
    c["mask"][seen] = 1
    masked = int(np.flatnonzero(c["mask"] == 0)[0])
    prior = c["prior"].copy()
    prior[seen] = value
    prior[masked] = value
    idx, score, count, flags = _call(c, k, "cosine", prior=prior, split=split)
    sees = np.array([seen not in c["idx"][c["ptr"][q]:c["ptr"][q + 1]] for q in c["queries"]])
    assert sees.any() and not sees.all()
    assert np.array_equal((flags & 2) != 0, sees) and not (flags & ~2).any()
    assert not np.isnan(score).any() and not (idx == masked).any()
    want = P.topk_prior(_s0(c, "cosine"), prior, c["queries"], k, c["ptr"], c["idx"], c["mask"])
    assert np.array_equal(want[3], sees)
    assert np.array_equal(idx, want[0]) and np.array_equal(_bits(score), _bits(want[1])) and np.array_equal(count, want[2])
    if value != value:
        assert not (idx == seen).any()  # a NaN is never returned
    else:
        assert (idx[sees, 0] == seen).all() and np.isposinf(score[sees, 0]).all()  # +inf orders as a value
    # a finite prior can overflow a finite inner product
    big = dict(c, qf=(c["qf"] * np.float32(1e19)), cand=(c["cand"] * np.float32(1e19)))
    assert (_call(big, k, "dot", prior=np.full(n_cand, 3e38, np.float32), split=split)[3] & 2).any()
    # the Python layer refuses before anything is uploaded
    tk = rank.TopK(c["ptr"], c["idx"], c["mask"], DEV)
    with pytest.raises(ValueError, match="not finite at candidate %d" % min(seen, masked)):
        tk.topk(_dev(c["qf"]), _dev(c["cand"]), c["queries"], k, prior=prior)
    assert tk._prior is None


# ------------------------------------------------------------------------------- 7. item stats and Gini
def _lists(seed, n, k, n_cand):
    """Lists of count 0, 1, k and random ones, -1 padded (never read); list 5 holds an out-of-range entry
    inside its count, list 6 one outside it."""
    rs = np.random.RandomState(seed)
    count = rs.randint(0, k + 1, n).astype(np.int32)
    count[:min(n, 3)] = [0, 1, k][:n]
    idx = np.full((n, k), -1, np.int32)
    for i in range(n):
        idx[i, :count[i]] = rs.choice(n_cand, count[i], replace=count[i] > n_cand)
    if n > 6:
        count[5] = max(count[5], 2)
        idx[5, :count[5]] = rs.choice(n_cand, count[5])
        idx[5, 1] = n_cand
        count[6] = 1
        idx[6, 0] = 0
        idx[6, 1:] = -5
    return idx, count


@pytest.mark.parametrize("n,k,n_cand,ks", [(3, 1, 1, (1,)), (9, 100, 65, (1, 10, 64, 65, 100)), (70, 128, 1000, (5, 128)),
                                           (1030, 10, 200, (1, 2, 3, 4, 5, 6, 7, 10))])
def test_item_stats_equal_the_sequential_loops(n, k, n_cand, ks):
    from dcrecommend.nn import rank
    idx, count = _lists(n + k, n, k, n_cand)
    rs = np.random.RandomState(n)
    value = -np.log2(rs.rand(n_cand) * 0.9 + 1e-3)
    tail = (rs.rand(n_cand) < 0.6).astype(np.uint8) * rs.randint(1, 255, n_cand).astype(np.uint8)
    didx, dcount = _dev(idx), _dev(count)
    for v, t in ((value, tail), (None, tail), (value, None), (None, None)):
        pop = rank.PopStats(DEV, n_cand, v, t)
        stats, flags = pop.stats_raw(didx, dcount, ks)
        want, wflags = P.item_stats(idx, count, list(ks), v, t, n_cand)
        assert np.array_equal(flags.cpu().numpy(), wflags)
        assert np.array_equal(stats.cpu().numpy().view(np.uint64), want.view(np.uint64))
        mean, n_eval = pop.mean_raw(stats, flags)
        wmean, wn = P.col_mean(want.reshape(n, -1), wflags)
        assert int(n_eval.cpu()[0]) == wn
        assert np.array_equal(mean.cpu().numpy().reshape(-1).view(np.uint64), wmean.view(np.uint64))
    # fed in two batches (the second not on a workgroup boundary): the same bits
    pop = rank.PopStats(DEV, n_cand, value, tail)
    whole, wf = pop.stats_raw(didx, dcount, ks)
    cut = n // 2 + 1
    a, af = pop.stats_raw(didx[:cut], dcount[:cut], ks)
    b, bf = (pop.stats_raw(didx[cut:], dcount[cut:], ks) if cut < n else (whole[:0], wf[:0]))
    assert torch.equal(torch.cat([a, b]), whole) and torch.equal(torch.cat([af, bf]), wf)
    assert torch.equal(pop.mean_raw(torch.cat([a, b]), torch.cat([af, bf]))[0], pop.mean_raw(whole, wf)[0])


def _exposure_of(idx, count, ks, n_cand):
    e = np.zeros((len(ks), n_cand), np.int32)
    for i in range(len(idx)):
        for j in range(min(count[i], ks[-1])):
            e[next(t for t, K in enumerate(ks) if j < K), idx[i, j]] += 1
    return e


@pytest.mark.parametrize("n_cand,m", [(1, 1), (65, 3), (1000, 8), (70000, 2)])
def test_gini_equals_the_sort_in_integers(n_cand, m):
    from dcrecommend.nn import rank
    rs = np.random.RandomState(n_cand)
    n_lists = 300
    pop = rank.PopStats(DEV, n_cand)
    # a popularity law: a few candidates hold most of the exposure, most hold none
    e = np.minimum(rs.zipf(1.6, (m, n_cand)) - 1, n_lists // m).astype(np.int32)
    e[:, rs.rand(n_cand) < 0.5] = 0
    mask = (rs.rand(n_cand) < 0.7).astype(np.uint8)
    mask[int(np.argmax(e.sum(0)))] = 0  # the mask removes the most exposed candidate
    for mk in (None, mask):
        g, total = pop.gini_raw(_dev(e), n_lists, _dev(mk))
        wg, wt = P.gini(e, mk)
        assert np.array_equal(total.cpu().numpy(), wt)
        assert np.array_equal(g.cpu().numpy().view(np.uint64), wg.view(np.uint64))
    # a larger histogram (another launch shape of the scan): the same bits
    g2, _ = pop.gini_raw(_dev(e), 50000, _dev(mask))
    assert torch.equal(g2, g)
    zero = np.zeros((m, n_cand), np.int32)
    assert not pop.gini(_dev(zero), n_lists).any()  # all-zero exposure
    one = zero.copy()
    one[0, n_cand // 2] = n_lists  # one candidate holds all of it: (n - 1) / n
    assert np.array_equal(pop.gini(_dev(one), n_lists), np.full(m, (n_cand - 1) / n_cand))
    flat = zero.copy()
    flat[-1, :] = 3  # equal exposure from the last cutoff on
    assert pop.gini(_dev(flat), n_lists)[-1] == 0.0 and not pop.gini(_dev(flat), n_lists)[:-1].any()
    # a count beyond the histogram, or a negative one, is refused, never an address
    one[0, n_cand // 2] = n_lists + 1
    assert (pop.gini_raw(_dev(one), n_lists)[1] == -1).all()
    with pytest.raises(ValueError, match="n_lists_max"):
        pop.gini(_dev(one), n_lists)
    one[0, n_cand // 2] = -1
    assert int(pop.gini_raw(_dev(one), n_lists)[1][0]) == -1


def test_gini_of_exposure_accumulated_in_two_batches():
    """dcue_topk_metrics' own exposure counts, the lists fed whole and in two batches: the same Gini bits, and
    the restatement's on the counts rebuilt from the lists."""
    from dcrecommend.nn import rank
    n, k, n_cand, ks = 70, 100, 200, (5, 50, 100)
    rs = np.random.RandomState(2)
    count = rs.randint(1, k + 1, n).astype(np.int32)
    idx = np.full((n, k), -1, np.int32)
    for i in range(n):
        idx[i, :count[i]] = (rs.zipf(1.4, count[i] * 4) % n_cand)[:count[i]]  # repeats allowed: positions count
    truth_ptr = np.arange(n + 1, dtype=np.int64)
    ev = rank.TopKMetrics(truth_ptr, np.zeros(n, np.int32), DEV, n_cand=n_cand)
    didx, dcount, q = _dev(idx), _dev(count), np.arange(n)
    whole = ev.new_exposure(len(ks))
    ev.metrics_raw(didx, dcount, q, ks, exposure=whole)
    parts = ev.new_exposure(len(ks))
    ev.metrics_raw(didx[:33], dcount[:33], q[:33], ks, exposure=parts)
    ev.metrics_raw(didx[33:], dcount[33:], q[33:], ks, exposure=parts)
    want = _exposure_of(idx, count, ks, n_cand)
    assert np.array_equal(whole.cpu().numpy(), want) and torch.equal(parts, whole)
    pop = rank.PopStats(DEV, n_cand)
    g = pop.gini(whole, n * k)  # (an index repeats within a list here: a count can pass the number of lists)
    assert np.array_equal(g.view(np.uint64), pop.gini(parts, n * k).view(np.uint64))
    assert np.array_equal(g.view(np.uint64), P.gini(want)[0].view(np.uint64))
    assert 0.0 < g[-1] < 1.0


# ------------------------------------------------------------------------------- 8. through the API
@pytest.fixture(scope="module")
def served(golden, tmp_path_factory):
    """The tiny trainer of the top-K tests (golden weights, factors computed on the GPU) with play counts:
    the training data's per-song user counts."""
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    train, val, items = _datasets(g, tmp_path_factory.mktemp("mel"))
    tr = DCUE(feature_dim=int(g["d"]), conv_hidden=int(g["H"]), batch_size=8, device=DEV)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    tr._init_nn()
    tr.model.load_state_dict({k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd.")})
    tr._user_factors(items)
    tr._item_factors(items)
    tr.train_data = train
    with pytest.raises(RuntimeError, match="set_popularity"):
        tr.recommend([g["val_users"][0]], popularity=0.5)
    tr.set_popularity()
    counts = np.asarray(train.item_user.tocsr().getnnz(axis=1))
    z, v, tail = tr._popularity_arrays(None)
    np.testing.assert_allclose(z, P.log_popularity(counts.tolist()), rtol=4e-16, atol=0)
    assert np.array_equal(tail, P.tail_bytes(counts.tolist()))
    users = [train.userindex2userid[int(r)] for r in tr._topk_metrics(None)[1]]
    return dict(g=g, tr=tr, train=train, val=val, users=users, z=z, v=v, tail=tail)


def _full_prior_ranking(s, rows, prior, exclude_seen=True):
    """The restatement's full ranking of every song for the user rows, on the library's own plain scores."""
    tr, train = s["tr"], s["train"]
    n = train.n_items
    c = dict(qf=tr.user_factors.cpu().numpy(), cand=tr._item_feat_by_index().cpu().numpy(), queries=np.asarray(rows),
             ptr=None, idx=np.zeros(0, np.int32), mask=None)
    s0 = _s0(c, "cosine")
    ptr, idx = train.user_item_csr() if exclude_seen else (None, None)
    return P.topk_prior(s0, prior, rows, n, ptr, idx, tr._cand_mask(None))


def test_recommend_with_popularity(served):
    s = served
    tr, train, users, z = s["tr"], s["train"], s["users"], s["z"]
    rows = np.array([train.user_index[u] for u in users])
    plain = tr.recommend(users, k=5, as_ids=False)
    for kw in (dict(popularity=0.0), dict(popularity=None, item_prior=None),
               dict(item_prior=np.zeros(train.n_items, np.float32))):
        got = tr.recommend(users, k=5, as_ids=False, **kw)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1]))
        assert np.array_equal(got[2], plain[2])
    assert tr.recommend(users[:3], k=5, popularity=0.0) == tr.recommend(users[:3], k=5)
    down = tr.recommend(users, k=5, as_ids=False, popularity=-1.0)
    up = tr.recommend(users, k=5, as_ids=False, popularity=1.0)
    assert (plain[2] == 5).all() and (down[2] == 5).all() and (up[2] == 5).all()
    mz = [float(z[lst[0]].mean()) for lst in (down, plain, up)]
    print("mean z of the served lists: popularity -1 %.4f, plain %.4f, +1 %.4f" % tuple(mz))
    assert mz[0] < mz[1] < mz[2]
    # exactly the restatement on the library's plain scores, and item_prior= is the same path
    for beta, got in ((-1.0, down), (1.0, up)):
        prior = (beta * z).astype(np.float32)
        want = _full_prior_ranking(s, rows, prior)
        assert np.array_equal(got[0], want[0][:, :5]) and np.array_equal(_bits(got[1]), _bits(want[1][:, :5]))
        same = tr.recommend(users, k=5, as_ids=False, item_prior=prior)
        assert np.array_equal(same[0], got[0]) and np.array_equal(_bits(same[1]), _bits(got[1]))
    with pytest.raises(ValueError, match="both"):
        tr.recommend(users, k=5, popularity=1.0, item_prior=np.zeros(train.n_items, np.float32))
    bad = np.zeros(train.n_items, np.float32)
    bad[3] = np.inf
    with pytest.raises(ValueError, match="not finite at candidate 3"):
        tr.recommend(users, k=5, item_prior=bad)
    # the other serving calls take the same prior
    why = tr.explain(users[:4], k=5, reasons=2, as_ids=False, popularity=-1.0)
    assert np.array_equal(why[0], down[0][:4]) and np.array_equal(_bits(why[1]), _bits(down[1][:4]))
    songs = [x for x in s["g"]["meta_songs"] if x in train.item_index]
    hist = [songs[:5], songs[7:10]]
    a = tr.recommend_for(hist, k=4, as_ids=False, steps=2, popularity=0.0)
    b = tr.recommend_for(hist, k=4, as_ids=False, steps=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    c = tr.recommend_for(hist, k=4, as_ids=False, steps=2, popularity=1.0)
    assert z[c[0]].mean() >= z[b[0]].mean()
    e = tr.explain_for(hist, k=4, reasons=2, as_ids=False, steps=2, popularity=1.0)
    assert np.array_equal(e[0], c[0]) and np.array_equal(_bits(e[1]), _bits(c[1]))


def test_capped_and_diverse_lists_carry_the_prior(served):
    from dcrecommend.nn import rank
    import group_reference as R
    s = served
    tr, train, users, z = s["tr"], s["train"], s["users"], s["z"]
    rows = np.array([train.user_index[u] for u in users])
    names = [train.itemindex2songid[i] for i in range(train.n_items)]
    tr.set_artists({song: ("BIG" if i % 4 else "A%d" % (i // 4 % 5)) for i, song in enumerate(names)})
    try:
        group_of = tr._artist_groups(None)[0]
        prior = (-1.0 * z).astype(np.float32)
        full = _full_prior_ranking(s, rows, prior)
        got = tr.recommend(users, k=4, as_ids=False, max_per_artist=1, pool=4, cap_rounds=16, popularity=-1.0)
        assert tr._topk("user", None, True).cap_rounds_used > 1  # deepening ran, with the prior in every round
        for r in range(len(users)):
            n = int(full[2][r])
            widx, wscore = R.cap_full_ranking(full[0][r, :n], full[1][r, :n], group_of, 1, 4)
            assert got[0][r, :got[2][r]].tolist() == list(widx), r
            assert np.array_equal(_bits(got[1][r, :got[2][r]]), _bits(wscore)), r
        # every song has an artist here, so the artist lists are the cap-1 song lists
        art = tr.recommend_artists(users[:5], k=3, popularity=-1.0)
        capped = tr.recommend(users[:5], k=3, max_per_artist=1, popularity=-1.0)
        assert [[(song, score) for _, song, score in a] for a in art] == capped
    finally:
        tr.set_artists(None)
    # diversity= with a prior: MMR over the prior pool, relevance min-max scaled
    tk = tr._topk("user", None, True)
    feat = tr._item_feat_by_index()
    pool = tk.topk_raw(tr.user_factors, feat, rows, 12, prior=prior)
    want = rank.Diversify(DEV).mmr_raw(pool[0], pool[1], pool[2], feat, 5, 0.5, "minmax")
    got = tr.recommend(users, k=5, as_ids=False, diversity=0.5, pool=12, popularity=-1.0)
    assert np.array_equal(got[0], want[0].cpu().numpy()) and np.array_equal(_bits(got[1]), _bits(want[1].cpu().numpy()))
    assert np.array_equal(got[2], want[2].cpu().numpy())
    raw = rank.Diversify(DEV).mmr_raw(pool[0], pool[1], pool[2], feat, 5, 0.5, "raw")
    explicit = tk.topk_raw(tr.user_factors, feat, rows, 5, diversity=0.5, pool=12, prior=prior, rel="raw")
    assert torch.equal(explicit[0], raw[0])  # an explicit rel still wins


def test_evaluate_topk_novelty_equals_the_restatement(served):
    s = served
    tr, train, users, v, tail = s["tr"], s["train"], s["users"], s["v"], s["tail"]
    ks = (2, 5)
    old = tr.evaluate_topk(ks=ks)
    assert tr.evaluate_topk(ks=ks, popularity=None, novelty=False) == old
    zero = tr.evaluate_topk(ks=ks, popularity=0.0)
    assert zero == old
    for beta in (None, -1.0):
        kw = {} if beta is None else dict(popularity=beta)
        new = tr.evaluate_topk(ks=ks, novelty=True, **kw)
        base = tr.evaluate_topk(ks=ks, **kw)
        extra = {"%s@%d" % (n, k) for n in ("novelty", "tail", "gini") for k in ks} | {"n_novelty"}
        assert set(new) == set(base) | extra and all(new[k] == base[k] for k in base)
        idx, _, count = tr.recommend(users, k=5, exclude_seen=False, as_ids=False, **kw)
        stats, flags = P.item_stats(idx.astype(np.int32), count, list(ks), v, tail, train.n_items)
        mean, ne = P.col_mean(stats.reshape(len(idx), -1), flags)
        assert new["n_novelty"] == ne == len(users)
        assert [new["novelty@2"], new["tail@2"], new["novelty@5"], new["tail@5"]] == mean.tolist()
        g, _ = P.gini(_exposure_of(idx, count, ks, train.n_items), tr._cand_mask(None))
        assert [new["gini@2"], new["gini@5"]] == g.tolist()
    demoted, plain = tr.evaluate_topk(ks=ks, novelty=True, popularity=-1.0), tr.evaluate_topk(ks=ks, novelty=True)
    print("novelty@5 %.4f -> %.4f, tail@5 %.4f -> %.4f, gini@5 %.4f -> %.4f under popularity = -1"
          % (plain["novelty@5"], demoted["novelty@5"], plain["tail@5"], demoted["tail@5"], plain["gini@5"],
             demoted["gini@5"]))


def test_wrmf_item_prior_and_novelty():
    from dcrecommend.dcbr.wrmf import WRMF
    rs = np.random.RandomState(4)
    n_users, n_items, f = 40, 300, 16
    m = WRMF(factors=f, device=DEV)  # factors set directly: serving needs no fit without exclude_seen
    m.user_factors, m.item_factors = _dev(rs.randn(n_users, f).astype(np.float32)), _dev(rs.randn(n_items, f).astype(np.float32))
    prior = rs.randn(n_items).astype(np.float32)
    users = np.arange(n_users)
    plain = m.recommend(users, k=10, exclude_seen=False)
    zero = m.recommend(users, k=10, exclude_seen=False, item_prior=np.zeros(n_items, np.float32))
    assert np.array_equal(plain[0], zero[0]) and np.array_equal(_bits(plain[1]), _bits(zero[1]))
    got = m.recommend(users, k=10, exclude_seen=False, item_prior=prior)
    c = dict(qf=m.user_factors.cpu().numpy(), cand=m.item_factors.cpu().numpy(), queries=users, ptr=None,
             idx=np.zeros(0, np.int32), mask=None)
    want = P.topk_prior(_s0(c, "dot"), prior, users, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    truth = [np.sort(rs.choice(n_items, 5, replace=False)) for _ in range(n_users)]
    tptr = np.arange(n_users + 1, dtype=np.int64) * 5
    tidx = np.concatenate(truth).astype(np.int32)
    value, tail = rs.rand(n_items), (rs.rand(n_items) < 0.5).astype(np.uint8)
    ks = (3, 10)
    old = m.evaluate_topk(tptr, tidx, ks=ks)
    new = m.evaluate_topk(tptr, tidx, ks=ks, item_prior=prior, item_value=value, item_tail=tail, gini=True)
    assert set(new) == set(old) | {"%s@%d" % (n, k) for n in ("novelty", "tail", "gini") for k in ks} | {"n_novelty"}
    stats, flags = P.item_stats(got[0].astype(np.int32), got[2], list(ks), value, tail, n_items)
    mean, ne = P.col_mean(stats.reshape(n_users, -1), flags)
    assert [new["novelty@3"], new["tail@3"], new["novelty@10"], new["tail@10"]] == mean.tolist() and new["n_novelty"] == ne
    assert [new["gini@3"], new["gini@10"]] == P.gini(_exposure_of(got[0], got[2], ks, n_items))[0].tolist()


def test_train_dcue_driver_writes_the_popularity_columns(tmp_path):
    import train_dcue
    out, metrics, counts = tmp_path / "rec.csv", tmp_path / "m.json", tmp_path / "counts.csv"
    pd.DataFrame({"song_id": ["S%07d" % i for i in range(0, 80, 2)], "count": np.arange(40) % 7}).to_csv(counts, index=False)
    argv = ["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80", "--synthetic-pairs", "300",
            "--feature-dim", "32", "--conv-hidden", "32", "--batch-size", "8", "--neg-batch-size", "3",
            "--num-epochs", "1", "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path / "ck"),
            "--recommend-k", "5", "--recommend-out", str(out), "--popularity", str(counts),
            "--recommend-popularity", "-0.5", "--eval-k", "2,5", "--eval-out", str(metrics), "--eval-novelty",
            "--eval-popularity", "-0.5"]
    dcue = train_dcue.main(argv)
    rec = pd.read_csv(out)
    assert list(rec.columns) == ["user_id", "rank", "song_id", "score"]
    users = list(dcue.train_data.uniq_users)
    want = dcue.recommend(users, k=5, popularity=-0.5)
    assert [list(g["song_id"]) for _, g in rec.groupby("user_id", sort=False)] == [[s for s, _ in lst] for lst in want]
    res = json.load(open(metrics))
    for split in ("val", "test"):
        for name in ("novelty", "tail", "gini", "ndcg"):
            assert all("%s@%d" % (name, k) in res[split] for k in (2, 5))
        assert res[split]["n_novelty"] == res[split]["n_users"] and 0.0 <= res[split]["gini@5"] <= 1.0
    with pytest.raises(SystemExit):
        train_dcue.parse(["--synthetic", "--recommend-popularity", "0.5"])
    with pytest.raises(SystemExit):
        train_dcue.parse(["--synthetic", "--eval-novelty"])
