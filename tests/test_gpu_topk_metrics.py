"""GPU tests of the top-K ranking metrics (dcue_topk_metrics / dcue_topk_metrics_mean, rank.TopKMetrics,
DCUE.evaluate_topk, train_dcue.py --eval-k) against the numpy restatement in topk_metrics_reference.py.

Tolerance: 1e-12 absolute per metric and per mean. At most 128 fp64 terms in [0, 1] are summed in
another order than the reference's (128 x 2^-53 = 1.4e-14), and the device's log2 is within an ulp or
two of the host's (relative 4e-16 on terms that sum to at most 21); both stay below about 1e-13.
Flags, n_evaluated and the exposure counts are integers and must be exact; coverage is a ratio of two
exact integers, compared to 1e-15.
"""
import functools
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import topk_metrics_reference as R
import topk_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
N_CAND = 70000
EDGE_ITEMS = (0, 65535, 65536, 69999)  # either side of 2^16, and both ends
N_PATTERNS, N_ROWS = 11, 21  # coprime: queries i < 231 meet every (pattern, truth row) pair


# ------------------------------------------------------------------------------- synthetic lists
def _cutoff_sets(k):
    """(1,), (k,), the lane-split set (1, 63, 64, 65, 128) cut to k, and eight cutoffs ending at k."""
    split = sorted({c for c in (1, 63, 64, 65, 128) if c < k} | {k})
    eight = sorted({c for c in (1, 2, 10, 63, 64, 65, 100) if c < k} | {k})
    return [(1,), (k,), tuple(split), tuple(eight)]


def _truth_rows(rs, ks):
    """21 sorted distinct rows: empty, 1, 2, exactly each cutoff, 129 and 3,000 items, the edge items,
    the rest 3..40 items."""
    sizes = [0, 1, 2, 129, 3000, -1] + sorted(set(ks) - {1, 2})
    sizes += [int(s) for s in rs.randint(3, 41, N_ROWS - len(sizes))]
    rows = [np.array(EDGE_ITEMS) if s < 0 else np.sort(rs.choice(N_CAND, s, replace=False)) for s in sizes]
    return [rows[i] for i in rs.permutation(N_ROWS)]


def _list(rs, pattern, truth, k, ks, i):
    """(list [k] of distinct items, count): where the list hits the truth row is the pattern's."""
    kap = ks[i % len(ks)]
    count = {5: 0, 6: 1, 7: kap - 1, 8: kap, 9: int(rs.randint(0, k + 1))}.get(pattern, k)
    if pattern == 0:
        want = np.ones(k, bool)  # everywhere
    elif pattern == 1:
        want = np.zeros(k, bool)  # nowhere
    elif pattern in (2, 6):
        want = np.arange(k) == 0  # position 0 only
    elif pattern == 3:
        want = np.isin(np.arange(k), (63, 64, 127))
    elif pattern == 10:
        want = np.arange(k) == 1  # the first hit is not the first entry
    else:
        want = rs.rand(k) < (0.2 if pattern == 9 else 0.5)
    other = rs.choice(N_CAND, k + len(truth), replace=False)
    other = other[~np.isin(other, truth)][:k]
    hits = rs.permutation(truth)[:int(want.sum())]  # truth items absent from the list remain
    want &= np.cumsum(want) <= len(hits)
    lst = other.copy()
    lst[want] = hits
    return lst, count


@functools.lru_cache(maxsize=None)
def _case(k, ks, n):
    """Lists, truth CSR and the reference's numbers for one (k, cutoffs, n_queries)."""
    rs = np.random.RandomState(1000 * k + 10 * n + len(ks))
    rows = _truth_rows(rs, ks)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    tidx = np.concatenate(rows).astype(np.int32)
    queries = np.arange(n) % N_ROWS  # every row, not in row order (the rows are permuted), with repeats
    lists = [_list(rs, i % N_PATTERNS, rows[queries[i]], k, ks, i) for i in range(n)]
    idx = np.stack([l for l, _ in lists]).astype(np.int32)
    count = np.array([c for _, c in lists], np.int32)
    padded = idx.copy()
    padded[np.arange(k)[None, :] >= count[:, None]] = -1
    expo = np.zeros((len(ks), N_CAND), np.int64)
    per, flags = R.metrics(padded, count, queries, ptr, tidx, list(ks), N_CAND, expo)
    c = dict(k=k, ks=ks, n=n, ptr=ptr, tidx=tidx, queries=queries, idx=padded, idx_filled=idx, count=count,
             per=per, flags=flags, expo=expo)
    _check_inputs(c)
    return c


def _check_inputs(c):
    """The conditions the inputs must meet, on the reference alone, before the GPU is consulted.
    A case of 257 queries meets every (pattern, row) pair, so it must show them all; the small cases
    (1 .. 5 queries) only add launch shapes. Which values a metric can take: hit is 0 or 1 at every
    cutoff; at cutoff 1 precision, NDCG, MAP and MRR are 0 or 1 too (one position: hit or not) and only
    recall (1 / t) lies in between; from cutoff 2 on every metric but hit can lie in (0, 1). Every
    metric reaches 1 at every cutoff (precision on a truth row of 129 or 3,000 items, the others on
    the 1-item row hit at position 0)."""
    if c["n"] < N_PATTERNS * N_ROWS:
        return
    ev = c["flags"] == 0
    assert ev.mean() >= 0.9 and not ev.all()
    per = c["per"][ev]
    for i, kap in enumerate(c["ks"]):
        for s in range(R.N_METRICS):
            v = per[:, i, s]
            assert (v == 0).any() and (v == 1).any(), (kap, R.NAMES[s])
            if s != R.HIT and (kap >= 2 or s == R.RECALL):
                assert ((v > 0) & (v < 1)).any(), (kap, R.NAMES[s])


def _evaluator(c, mask=None):
    from dcrecommend.nn import rank
    return rank.TopKMetrics(c["ptr"], c["tidx"], DEV, cand_mask=mask, n_cand=None if mask is not None else N_CAND)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raw(ev, c, idx=None, exposure=None):
    per, flags = ev.metrics_raw(_dev(c["idx"] if idx is None else idx), _dev(c["count"]), c["queries"], c["ks"],
                                exposure=exposure)
    return per.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 127, 128])
def test_synthetic_lists(k, n):
    for ks in _cutoff_sets(k):
        c = _case(k, ks, n)
        ev = _evaluator(c)
        per, flags = _raw(ev, c)
        assert per.shape == (n, len(ks), 6) and per.dtype == np.float64
        assert np.array_equal(flags, c["flags"])
        err = np.abs(per - c["per"]).max()
        print("k %d ks %s n %d: max |metric - reference| %.3e" % (k, ks, n, err))
        assert err <= TOL
        # whatever stands past `count` is never looked at
        per2, flags2 = _raw(ev, c, idx=c["idx_filled"])
        assert np.array_equal(per2, per) and np.array_equal(flags2, flags)


def test_edge_items_hit():
    """Hits at candidates 0, 65,535, 65,536 and 69,999 of 70,000."""
    c = _case(128, (1, 63, 64, 65, 128), 257)
    row = next(r for r in range(N_ROWS) if c["ptr"][r + 1] - c["ptr"][r] == 4
               and tuple(c["tidx"][c["ptr"][r]:c["ptr"][r + 1]]) == EDGE_ITEMS)
    q = next(i for i in range(c["n"]) if c["queries"][i] == row and i % N_PATTERNS == 0)
    assert set(EDGE_ITEMS) <= set(c["idx"][q].tolist()) and c["per"][q, -1, R.RECALL] == 1.0
    per, _ = _raw(_evaluator(c), c)
    assert abs(per[q] - c["per"][q]).max() <= TOL and per[q, -1, R.RECALL] == 1.0


# ------------------------------------------------------------------------------- out of range
def test_out_of_range_entries_are_flagged_and_left_out():
    c = _case(128, (1, 63, 64, 65, 128), 257)
    ev = _evaluator(c)
    ok = np.flatnonzero((c["flags"] == 0) & (c["count"] > 5))
    qa, qb = int(ok[3]), int(ok[40])
    idx = c["idx"].copy()
    idx[qa, 3] = N_CAND
    idx[qb, 0] = -5
    expo_clean, expo_bad = ev.new_exposure(5), ev.new_exposure(5)
    per0, flags0 = _raw(ev, c, exposure=expo_clean)
    per1, flags1 = _raw(ev, c, idx=idx, exposure=expo_bad)
    want_flags = c["flags"].copy()
    want_flags[[qa, qb]] |= 2
    assert np.array_equal(flags1, want_flags) and np.array_equal(flags0, c["flags"])
    assert np.all(per1[[qa, qb]] == 0)
    rest = np.ones(c["n"], bool)
    rest[[qa, qb]] = False
    assert np.array_equal(per1[rest], per0[rest])  # bit for bit
    expo = np.zeros((5, N_CAND), np.int64)
    ref_per, ref_flags = R.metrics(idx, c["count"], c["queries"], c["ptr"], c["tidx"], list(c["ks"]), N_CAND, expo)
    assert np.array_equal(ref_flags, want_flags)
    assert np.array_equal(expo_bad.cpu().numpy(), expo) and np.array_equal(expo_clean.cpu().numpy(), c["expo"])
    assert not np.array_equal(expo, c["expo"])
    mean, cov, n_eval = ev.mean_raw(_dev(per1), _dev(flags1), expo_bad)
    ref_mean, ref_n = R.means(ref_per, ref_flags)
    assert int(n_eval.cpu()[0]) == ref_n == int((c["flags"] == 0).sum()) - 2
    assert np.abs(mean.cpu().numpy() - ref_mean).max() <= TOL
    assert np.abs(cov.cpu().numpy() - R.coverage(expo, None, N_CAND)).max() <= 1e-15


# ------------------------------------------------------------------------------- exposure, coverage
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k,n", [(1, 5), (64, 257), (65, 257), (128, 257), (128, 3)])
def test_exposure_and_coverage(k, n, masked):
    mask = (np.random.RandomState(k + n).rand(N_CAND) < 0.8).astype(np.uint8) if masked else None
    for ks in _cutoff_sets(k):
        c = _case(k, ks, n)
        ev = _evaluator(c, mask)
        expo = ev.new_exposure(len(ks))
        per, flags = _raw(ev, c, exposure=expo)
        assert np.array_equal(expo.cpu().numpy(), c["expo"])
        mean, cov, n_eval = ev.mean_raw(_dev(per), _dev(flags), expo)
        want_cov = R.coverage(c["expo"], mask, N_CAND)
        assert np.abs(cov.cpu().numpy() - want_cov).max() <= 1e-15
        assert int(n_eval.cpu()[0]) == int((c["flags"] == 0).sum())
        assert np.abs(mean.cpu().numpy() - R.means(c["per"], c["flags"])[0]).max() <= TOL
        # a second call accumulates: the counts double, coverage stays
        _raw(ev, c, exposure=expo)
        assert np.array_equal(expo.cpu().numpy(), 2 * c["expo"])
        assert np.array_equal(ev.mean_raw(_dev(per), _dev(flags), expo)[1].cpu().numpy(), cov.cpu().numpy())
        # without exposure there is no coverage
        assert ev.mean_raw(_dev(per), _dev(flags))[1] is None


# ------------------------------------------------------------------------------- the mean
@pytest.mark.parametrize("ks", [(1, 63, 64, 65, 128), (1, 2, 10, 63, 64, 65, 100, 128), (128,)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 10000])
def test_mean_reduction(n, ks):
    c = _case(128, ks, 257)
    ev = _evaluator(c)
    m = len(ks)
    rep = np.arange(n) % 257
    idx, count, q = _dev(c["idx"][rep]), _dev(c["count"][rep]), _dev(c["queries"][rep].astype(np.int32))
    cut = ev._cutoffs(ks)[1]
    means = []
    for batch in (n, 1, 5, 4096):
        per = torch.zeros((n, m, 6), dtype=torch.float64, device=DEV)
        flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        for q0 in range(0, n, batch):
            q1 = min(n, q0 + batch)
            ev._metrics_into(idx[q0:q1], count[q0:q1], q[q0:q1], cut, m, per[q0:], flags[q0:], None)
        mean, cov, n_eval = ev.mean_raw(per, flags)
        means.append((mean.cpu().numpy(), int(n_eval.cpu()[0])))
        if batch == n:
            per_h, flags_h = per.cpu().numpy(), flags.cpu().numpy()
            assert np.array_equal(flags_h, c["flags"][rep])
            assert np.abs(per_h - c["per"][rep]).max() <= TOL
    keep = flags_h == 0
    want = np.mean(per_h[keep], axis=0) if keep.any() else np.zeros((m, 6))
    err = np.abs(means[0][0] - want).max()
    print("n %d m %d: max |mean - np.mean| %.3e" % (n, m, err))
    assert err <= TOL and means[0][1] == int(keep.sum())
    assert np.abs(means[0][0] - R.means(c["per"][rep], c["flags"][rep])[0]).max() <= TOL
    for got in means[1:]:
        assert np.array_equal(got[0], means[0][0]) and got[1] == means[0][1]


def test_mean_of_nothing():
    c = _case(128, (128,), 257)
    ev = _evaluator(c)
    mean, cov, n_eval = ev.mean_raw(torch.zeros((0, 1, 6), dtype=torch.float64, device=DEV),
                                    torch.zeros(0, dtype=torch.int32, device=DEV), ev.new_exposure(1))
    assert np.all(mean.cpu().numpy() == 0) and int(n_eval.cpu()[0]) == 0 and np.all(cov.cpu().numpy() == 0)
    per, flags = ev.metrics_raw(torch.zeros((0, 4), dtype=torch.int32, device=DEV),
                                torch.zeros(0, dtype=torch.int32, device=DEV), [], (1, 4))
    assert tuple(per.shape) == (0, 2, 6) and flags.numel() == 0


# ------------------------------------------------------------------------------- end to end
def _lattice(rs, n, d):
    """Rows of 16 entries +-1: norm exactly 4, every cosine a multiple of 1/16, exact in fp32 in any
    summation order, so ties break by index exactly as the fp64 reference selects."""
    x = np.zeros((n, d), np.float32)
    for r in range(n):
        x[r, rs.choice(d, 16, replace=False)] = rs.choice(np.array([-1.0, 1.0], np.float32), 16)
    return x


def _random_csr(rs, n_rows, n_cand, max_len):
    rows = [np.sort(rs.choice(n_cand, rs.randint(0, max_len + 1), replace=False)) for _ in range(n_rows)]
    return rows


def _csr(rows):
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            np.concatenate(rows).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _e2e(d, lattice):
    n_rows, n_cand, n_queries = 130, 2500, 150
    rs = np.random.RandomState(17 + d + lattice)
    cand = _lattice(rs, n_cand, d) if lattice else rs.randn(n_cand, d).astype(np.float32)
    dup = rs.choice(n_cand, n_cand // 20, replace=False)
    cand[dup] = cand[rs.choice(n_cand, len(dup))]  # exact ties
    cand[rs.choice(n_cand, 3, replace=False)] = 0.0
    qf = _lattice(rs, n_rows, d) if lattice else rs.randn(n_rows, d).astype(np.float32)
    qf[5] = qf[9]
    qf[11] = 0.0
    mask = (rs.rand(n_cand) < 0.8).astype(np.uint8)
    excl_ptr, excl_idx = _csr(_random_csr(rs, n_rows, n_cand, 60))
    all_scores = T.cosines(qf, cand, np.arange(n_rows))
    truth = []
    for r in range(n_rows):
        t = rs.randint(0, 41)
        best = np.argsort(-all_scores[r], kind="stable")[:200]
        truth.append(np.unique(np.concatenate([rs.choice(best, t // 2, replace=False),
                                               rs.choice(n_cand, t - t // 2, replace=False)])))
    truth[3] = np.zeros(0, np.int64)
    tptr, tidx = _csr(truth)
    queries = rs.randint(0, n_rows, n_queries)
    queries[:2] = (3, 11)
    return dict(qf=qf, cand=cand, mask=mask, excl_ptr=excl_ptr, excl_idx=excl_idx, tptr=tptr, tidx=tidx,
                queries=queries, s64=all_scores[queries], n_cand=n_cand)


def _e2e_evaluator(c):
    from dcrecommend.nn import rank
    return rank.TopKMetrics(c["tptr"], c["tidx"], DEV, excl_ptr=c["excl_ptr"], excl_idx=c["excl_idx"],
                            cand_mask=c["mask"])


def _assert_result(res, ks, idx, count, c):
    """`res` of TopKMetrics.evaluate against the reference's numbers for the lists idx / count."""
    expo = np.zeros((len(ks), c["n_cand"]), np.int64)
    per, flags = R.metrics(idx, count, c["queries"], c["tptr"], c["tidx"], list(ks), c["n_cand"], expo)
    mean, n_eval = R.means(per, flags)
    assert res["ks"] == list(ks) and res["n_evaluated"] == n_eval and 0 < n_eval < len(flags)
    assert np.array_equal(res["flags"], flags)
    assert np.abs(res["per_query"] - per).max() <= TOL
    assert per.max() > 0, "no hit anywhere: the case checks nothing"
    for s, name in enumerate(R.NAMES):
        assert res[name].shape == (len(ks),) and res[name].dtype == np.float64
        assert np.abs(res[name] - mean[:, s]).max() <= TOL, name
    assert np.abs(res["coverage"] - R.coverage(expo, c["mask"], c["n_cand"])).max() <= 1e-15


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("d", [100, 128])
def test_end_to_end_exact_scores(d):
    c = _e2e(d, True)
    ks = (1, 10, 100)
    ev = _e2e_evaluator(c)
    qf, cand = _dev(c["qf"]), _dev(c["cand"])
    first = ev.evaluate(qf, cand, c["queries"], ks, per_query=True)
    idx, _, count = T.topk(None, None, c["queries"], 100, c["excl_ptr"], c["excl_idx"], c["mask"], scores=c["s64"])
    _assert_result(first, ks, idx, count, c)
    for qb in (1, 7, 64):
        _same(ev.evaluate(qf, cand, c["queries"], ks, query_batch=qb, per_query=True), first)
    # cutoffs in any order, with repeats
    _same(ev.evaluate(qf, cand, c["queries"], (100, 1, 10, 10), per_query=True), first)
    assert "per_query" not in ev.evaluate(qf, cand, c["queries"], ks)


def test_end_to_end_gaussian():
    c = _e2e(128, False)
    ks = (10, 50)
    ev = _e2e_evaluator(c)
    qf, cand = _dev(c["qf"]), _dev(c["cand"])
    res = ev.evaluate(qf, cand, c["queries"], ks, per_query=True)
    # fp32 near-ties may order differently from fp64: the oracle is the reference on the GPU's own lists
    idx, _, count = ev.topk.topk(qf, cand, c["queries"], 50)
    _assert_result(res, ks, idx, count, c)


def test_non_finite_factors_raise():
    c = _e2e(128, False)
    ev = _e2e_evaluator(c)
    cand = c["cand"].copy()
    cand[int(np.flatnonzero(c["mask"])[7])] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN"):
        ev.evaluate(_dev(c["qf"]), _dev(cand), c["queries"], (10, 50))


# ------------------------------------------------------------------------------- trainer
def _datasets(g, tmp_path):
    from dcrecommend.datasets.dcuepredset import DCUEPredset
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    trip = pd.DataFrame({"user_id": g["raw_users"], "song_id": g["raw_songs"], "score": g["raw_score"]})
    paths = []
    for k in range(len(g["meta_songs"])):
        p = os.path.join(str(tmp_path), "m%03d.pt" % k)
        torch.save(torch.from_numpy(g["spec"][k].astype(np.float32)), p)
        paths.append(p)
    meta = pd.DataFrame({"idx": np.arange(len(g["meta_songs"])), "song_id": g["meta_songs"], "data_mel": paths})
    return (DCUEPredset(trip.copy(), meta, split="train"), DCUEPredset(trip.copy(), meta, split="val"),
            DCUEItemset(trip.copy(), meta))


@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    train, val, items = _datasets(g, tmp_path_factory.mktemp("mel"))
    tr = DCUE(feature_dim=int(g["d"]), conv_hidden=int(g["H"]), batch_size=8, device=DEV)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    tr._init_nn()
    tr.model.load_state_dict({k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd.")})
    with pytest.raises(RuntimeError, match="no factors"):
        tr.evaluate_topk(val)
    tr._user_factors(items)
    tr._item_factors(items)
    with pytest.raises(RuntimeError, match="needs the interactions"):
        tr.evaluate_topk()  # no dataset given and none bound by fit()
    tr.train_data = train
    return g, tr, train, val, items


def _truth_by_user(ds, candidates, audio):
    """{user index: sorted candidate items the user interacted with in any split}, from the
    item x user matrix itself."""
    cand = set(int(i) for i in candidates if int(i) in audio)
    out = {}
    for ui in range(ds.n_users):
        items = sorted(int(i) for i in ds.item_user.getcol(ui).nonzero()[0] if int(i) in cand)
        if items:
            out[ui] = items
    return out


def test_evaluate_topk_matches_recommend(trained):
    g, tr, train, val, items = trained
    ks = (1, 5, 10)
    audio = {val.item_index[s] for s in g["meta_songs"] if s in val.item_index}
    truth = _truth_by_user(val, val.split_items(), audio)
    assert len(truth) >= 3
    res = tr.evaluate_topk(val, ks=ks, per_user=True)
    users = [val.userindex2userid[ui] for ui in sorted(truth)]
    assert res["users"] == users and res["n_users"] == len(users)  # exactly the users with truth
    idx, score, count = tr.recommend(users, k=10, dataset=val, exclude_seen=False, as_ids=False)
    rows = [np.array(truth.get(ui, []), np.int64) for ui in range(val.n_users)]
    tptr, tidx = _csr(rows)
    expo = np.zeros((3, val.n_items), np.int64)
    per, flags = R.metrics(idx, count, sorted(truth), tptr, tidx, list(ks), val.n_items, expo)
    assert not flags.any() and np.array_equal(res["flags"], flags)
    assert np.abs(res["per_user"] - per).max() <= TOL
    mean, _ = R.means(per, flags)
    n_candidates = len([i for i in val.split_items() if int(i) in audio])
    seen = np.zeros(val.n_items, bool)
    for i, k in enumerate(ks):
        for s, name in enumerate(R.NAMES):
            assert abs(res["%s@%d" % (name, k)] - mean[i, s]) <= TOL
        seen |= expo[i] != 0
        assert abs(res["coverage@%d" % k] - seen.sum() / n_candidates) <= 1e-15
    assert set(res) == {"%s@%d" % (n, k) for n in R.NAMES + ("coverage",) for k in ks} | {
        "n_users", "users", "per_user", "flags"}
    # chosen users, in the caller's order; one without truth is flagged and left out
    some = [users[2], users[0]]
    sub = tr.evaluate_topk(val, ks=ks, users=some, per_user=True)
    assert sub["users"] == some and np.array_equal(sub["per_user"], res["per_user"][[2, 0]])
    assert sub["n_users"] == 2
    with pytest.raises(KeyError):
        tr.evaluate_topk(val, ks=ks, users=["no such user"])
    with pytest.raises(ValueError, match=r"1\.\.128"):
        tr.evaluate_topk(val, ks=(0,))


def test_evaluate_topk_without_dataset(trained):
    g, tr, train, val, items = trained
    audio = {train.item_index[s] for s in g["meta_songs"] if s in train.item_index}
    truth = _truth_by_user(train, range(train.n_items), audio)
    res = tr.evaluate_topk(ks=(1, 5))
    assert res["n_users"] == len(truth) > 0
    assert set(res) == {"%s@%d" % (n, k) for n in R.NAMES + ("coverage",) for k in (1, 5)} | {"n_users"}
    assert all(0.0 <= float(v) <= 1.0 for key, v in res.items() if key != "n_users")


# ------------------------------------------------------------------------------- driver
def test_train_dcue_driver_writes_metrics(tmp_path):
    import train_dcue
    out = tmp_path / "m.json"
    argv = ["--synthetic", "--num-epochs", "1", "--save-dir", str(tmp_path / "ck"), "--eval-k", "1,5"]
    with pytest.raises(SystemExit):
        train_dcue.parse(argv)  # --eval-k without --eval-out
    with pytest.raises(SystemExit):
        train_dcue.parse(argv[:-2] + ["--eval-out", str(out)])
    train_dcue.main(argv + ["--eval-out", str(out)])
    res = json.loads(out.read_text())
    assert set(res) == {"val", "test"}
    want = {"%s@%d" % (n, k) for n in R.NAMES + ("coverage",) for k in (1, 5)} | {"n_users"}
    for split in ("val", "test"):
        assert set(res[split]) == want
        assert res[split]["n_users"] > 0
        for key, v in res[split].items():
            if key != "n_users":
                assert np.isfinite(v) and 0.0 <= v <= 1.0, (split, key, v)
