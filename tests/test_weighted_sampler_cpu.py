"""Popularity-weighted catalogue negatives, host side: the tables of datasets/csr.py with the
two-search mapping the kernel evaluates (restated in numpy here), popularity_weights and the dataset's
host path, against the definition in weighted_sampler_reference.py. Integers only: every comparison
is exact."""
import numpy as np
import pandas as pd
import pytest

import weighted_sampler_reference as R

MAXW = 2 ** 32 - 1


def _mapped(tables, indptr, u, r):
    """The kernel's evaluation of a draw: e* = #{e : K_e <= r}, g = r + E_{e*}, position = #{q : C[q+1] <= g}."""
    cum, key, skip, user_weight = (np.asarray(a).astype(np.int64) for a in tables)
    rb, re = int(indptr[u]), int(indptr[u + 1])
    e = np.searchsorted(key[rb:re], r, side='right')
    E = np.concatenate([skip[rb:re], [cum[-1] - user_weight[u]]])
    return np.searchsorted(cum[1:], r + E[e], side='right')


def _sample_mapped(seed, split, tables, indptr, users, N):
    rs = np.random.RandomState(seed)
    out = np.empty((len(users), N), dtype=np.int64)
    for i, u in enumerate(users):
        wu = int(tables[3][u])
        if wu == 0:
            out[i] = -1
            continue
        out[i] = split[_mapped(tables, indptr, u, rs.randint(0, wu, N))]
    return out, rs


def _case(seed, n=257, n_users=120, scale=1, total=None):
    """Random users over n split positions: 20 % zero weights, zero-weight runs at both ends, users with
    no split items, and users 0..3 = (every positive position: W_u == 0; all but one position of weight
    1: W_u == 1; no items; the first and last positive positions)."""
    rs = np.random.RandomState(seed)
    split = np.sort(rs.choice(3 * n, n, replace=False)).astype(np.int64)
    w = rs.randint(1, 50, n).astype(np.int64) * scale
    w[rs.rand(n) < 0.2] = 0
    w[:5] = 0
    w[-7:] = 0
    one = int(rs.choice(np.nonzero(w)[0]))
    w[one] = 1
    if total is not None:  # an exact total: the spare goes to one position
        big = int(np.nonzero(w)[0][3])
        w[big] += total - int(w.sum())
        assert w[big] > 0
    pos = np.nonzero(w)[0]
    lists = [pos, pos[pos != one], np.zeros(0, np.int64), pos[[0, -1]]]
    for u in range(4, n_users):
        k = 0 if u % 9 == 0 else int(rs.randint(1, n // 2))
        lists.append(np.sort(rs.choice(n, k, replace=False)))
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ranks = np.concatenate(lists).astype(np.int32)
    users = rs.randint(0, n_users, 300).astype(np.int64)
    users[[0, 5, 77, 150, 299]] = [1, 0, 2, 3, 1]
    return split, w, indptr, ranks, users


@pytest.mark.parametrize("kind", ["small", "large", "exact_max", "unit"])
@pytest.mark.parametrize("N", [1, 20])
def test_tables_and_mapping_equal_the_definition(kind, N):
    from dcrecommend.datasets.csr import weighted_saturated_users, weighted_split_tables
    if kind == "small":
        split, w, indptr, ranks, users = _case(1)
    elif kind == "large":  # W in (2^31, 2^32 - 1]: the mask is all ones
        split, w, indptr, ranks, users = _case(2, scale=650000)
        assert 2 ** 31 < int(w.sum()) <= MAXW
    elif kind == "exact_max":
        split, w, indptr, ranks, users = _case(3, scale=400000, total=MAXW)
        assert int(w.sum()) == MAXW
    else:
        split, w, indptr, ranks, users = _case(4)
        w = np.ones_like(w)
    tables = weighted_split_tables(indptr, ranks, w)
    assert all(t.dtype == np.uint32 for t in tables)
    assert len(tables[0]) == len(w) + 1 and len(tables[1]) == len(tables[2]) == len(ranks)
    assert int(tables[0][-1]) == int(w.sum())
    for u in range(len(indptr) - 1):  # K is non-decreasing within a list
        assert (np.diff(tables[1][indptr[u]:indptr[u + 1]].astype(np.int64)) >= 0).all()
    if kind != "unit":
        assert int(tables[3][0]) == 0 and int(tables[3][1]) == 1 and int(tables[3][2]) == int(w.sum())
        assert list(weighted_saturated_users(tables[3])) == [0]
    got, rs = _sample_mapped(11, split, tables, indptr, users, N)
    want = R.sample_users(11, False, split, w, indptr, ranks, users, N)
    assert np.array_equal(got, want)
    if kind != "unit":
        assert (got[5] == -1).all() and (got != -1)[users != 0].all()
        assert not np.isin(got[users != 0], split[w == 0]).any()  # a zero-weight song is never drawn
    # the same number of draws consumed: the streams continue alike
    ref = np.random.RandomState(11)
    for u in users:
        R.sample(ref, split, w, ranks[indptr[u]:indptr[u + 1]], N)
    assert ref.randint(0, 2 ** 31) == rs.randint(0, 2 ** 31)


def test_unit_weights_are_the_uniform_sampler():
    """w == 1: the draw is np.random.choice(nonitems, N)'s, value and stream position."""
    from dcrecommend.datasets.csr import weighted_split_tables
    split, _, indptr, ranks, users = _case(6)
    tables = weighted_split_tables(indptr, ranks, np.ones(len(split), dtype=np.int64))
    got, rs = _sample_mapped(3, split, tables, indptr, users, 7)
    ref = np.random.RandomState(3)
    for i, u in enumerate(users):
        keep = np.ones(len(split), dtype=bool)
        keep[ranks[indptr[u]:indptr[u + 1]]] = False
        assert np.array_equal(got[i], ref.choice(split[keep], 7))
    assert ref.randint(0, 2 ** 31) == rs.randint(0, 2 ** 31)


def test_table_errors():
    from dcrecommend.datasets.csr import weighted_split_tables
    indptr, ranks = np.array([0, 2, 3]), np.array([0, 2, 1], dtype=np.int32)
    weighted_split_tables(indptr, ranks, np.array([1, 0, 5]))
    with pytest.raises(ValueError, match="negative"):
        weighted_split_tables(indptr, ranks, np.array([1, -1, 5]))
    with pytest.raises(ValueError, match="mismatch"):
        weighted_split_tables(indptr, ranks, np.array([1, 1]))           # rank 2 has no weight
    with pytest.raises(ValueError, match="mismatch"):
        weighted_split_tables(np.array([0, 2, 4]), ranks, np.array([1, 1, 1]))  # indptr past the ranks
    with pytest.raises(ValueError, match="2\\^32"):
        weighted_split_tables(indptr, ranks, np.array([2 ** 31, 2 ** 31, 0]))
    with pytest.raises(ValueError, match="2\\^32"):
        weighted_split_tables(indptr, ranks, np.array([2 ** 40, 0, 0]))
    with pytest.raises(ValueError):
        weighted_split_tables(indptr, ranks, np.array([1.0, 2.0, 3.0]))
    assert int(weighted_split_tables(indptr, ranks, np.array([2 ** 31, 2 ** 31 - 1, 0]))[0][-1]) == MAXW


def test_popularity_weights():
    from dcrecommend.datasets.csr import popularity_weights
    rs = np.random.RandomState(0)
    counts = rs.randint(1, 1000, 500)
    w = popularity_weights(counts, 0.0)
    assert w.dtype == np.uint32 and (w == 1).all()
    assert (popularity_weights(np.full(9, 17), 0.75) == 1).all()  # all equal: the uniform sampler
    assert len(popularity_weights(np.zeros(0, np.int64), 0.75)) == 0
    # a small catalogue (100 songs x at most 49^0.75 x 2^20 < 2^31): S = 2^20, w = floor(count^alpha * 2^20)
    counts = rs.randint(1, 50, 100)
    w = popularity_weights(counts, 0.75)
    assert np.array_equal(w, np.floor(counts.astype(np.float64) ** 0.75 * 2 ** 20).astype(np.uint32))
    assert np.array_equal(w, popularity_weights(counts.copy(), 0.75))
    # 10^6 songs with counts up to 10^6: within the bound, at the largest power of two that is
    for counts in (rs.randint(1, 10 ** 6 + 1, 10 ** 6), np.minimum(rs.zipf(1.3, 10 ** 6), 10 ** 6)):
        counts[:2] = [1, 10 ** 6]
        w = popularity_weights(counts, 0.75)
        f = counts.astype(np.float64) ** 0.75
        assert w.dtype == np.uint32 and w.min() >= 1 and int(w.astype(np.uint64).sum()) <= MAXW
        # the largest power of two, at most 2^20, within the bound (floors below 2^36: the uint64 sum is exact)
        S = next(2.0 ** k for k in range(20, -41, -1)
                 if int(np.floor(f * 2.0 ** k).astype(np.uint64).sum()) + len(f) <= MAXW)
        assert S < 2 ** 20
        assert np.array_equal(w, np.maximum(1, np.floor(f * S)).astype(np.uint32))
        order = np.argsort(counts, kind="stable")
        assert (np.diff(w[order].astype(np.int64)) >= 0).all()  # monotone in the count
    with pytest.raises(ValueError, match="alpha"):
        popularity_weights(counts, -0.5)
    with pytest.raises(ValueError, match="alpha"):
        popularity_weights(counts, float("nan"))
    with pytest.raises(ValueError, match="count"):
        popularity_weights(np.array([3, 0, 2]), 0.75)


def _frames(seed=4, n_users=40, n_songs=90, n_pairs=700):
    rs = np.random.RandomState(seed)
    pairs = set()
    while len(pairs) < n_pairs:  # heavy-tailed songs
        pairs.add((int(rs.randint(n_users)), int(min(n_songs - 1, rs.zipf(1.4) - 1))))
    pairs |= {(0, s) for s in range(n_songs)}  # user 0 has every song: no candidate in any split
    pairs = sorted(pairs)
    trip = pd.DataFrame({"user_id": ["u%03d" % u for u, _ in pairs], "song_id": ["S%03d" % s for _, s in pairs],
                         "score": rs.randint(1, 9, len(pairs))})
    songs = sorted(set(trip["song_id"]))
    meta = pd.DataFrame({"idx": np.arange(len(songs)), "song_id": songs, "data_mel": [""] * len(songs)})
    return trip, meta


def _user_ranks(ds, user_id, split):
    items = ds.item_user.getcol(ds.user_index[user_id]).nonzero()[0]
    return np.nonzero(np.isin(split, items))[0]


@pytest.mark.parametrize("mode", ["popularity", "weights"])
def test_dataset_host_path_equals_the_definition(mode):
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    state = np.random.get_state()
    try:
        trip, meta = _frames()
        kw = {}
        if mode == "weights":
            kw["neg_weights"] = np.random.RandomState(1).randint(0, 4, trip["song_id"].nunique()) * 1000
        ds = DCUEDataset(trip.copy(), meta, neg_samples=6, split="train", neg_sampling=mode, **kw)
        split, w = ds.split_items(), ds.negative_weights()
        assert w.dtype == np.uint32 and len(w) == len(split)
        if mode == "popularity":
            counts = np.array([ds.item_user.getrow(i).nnz for i in split])
            assert np.array_equal(w, np.floor(counts.astype(np.float64) ** 0.75 * 2 ** 20).astype(np.uint32))
            assert len(set(w.tolist())) > 3
        else:
            assert np.array_equal(w, kw["neg_weights"][split]) and (w == 0).any()
        users = [u for u in ds.uniq_users if u != "u000"][:25]
        np.random.seed(21)
        got = [ds._user_nonitem_songids(u) for u in users]
        after = np.random.randint(0, 2 ** 31)
        np.random.seed(21)
        for u, names in zip(users, got):
            want = R.sample(np.random, split, w, _user_ranks(ds, u, split), 6)
            assert [ds.item_index[s] for s in names] == want.tolist()
        assert np.random.randint(0, 2 ** 31) == after
        with pytest.raises(ValueError):  # no candidate: numpy's randint(0, 0)
            ds._user_nonitem_songids("u000")
    finally:
        np.random.set_state(state)


def test_dataset_uniform_is_unchanged():
    """'uniform', the default: the reference's draw (datasets/dcuedataset.py:207-220), value and stream."""
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    state = np.random.get_state()
    try:
        trip, meta = _frames()
        ds = DCUEDataset(trip.copy(), meta, neg_samples=6, split="train")
        assert ds.neg_sampling == "uniform" and (ds.negative_weights() == 1).all()
        explicit = DCUEDataset(trip.copy(), meta, neg_samples=6, split="train", neg_sampling="uniform", neg_alpha=0.3)
        users = [u for u in ds.uniq_users if u != "u000"][:25]
        np.random.seed(8)
        got = [ds._user_nonitem_songids(u) for u in users]
        after = np.random.get_state()
        np.random.seed(8)
        assert [explicit._user_nonitem_songids(u) for u in users] == got
        np.random.seed(8)
        for u, names in zip(users, got):
            items = ds.item_user.getcol(ds.user_index[u]).nonzero()[0]
            non = ds.all_items[(~np.isin(ds.all_items, items)) & np.isin(ds.all_items, ds.uniq_song_idxs)]
            assert [ds.item_index[s] for s in names] == np.random.choice(non, 6).tolist()
        mine = np.random.get_state()
        assert np.array_equal(after[1], mine[1]) and after[2] == mine[2]
    finally:
        np.random.set_state(state)


def test_dataset_argument_errors():
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    state = np.random.get_state()
    try:
        trip, meta = _frames()
        n = trip["song_id"].nunique()
        with pytest.raises(ValueError, match="neg_sampling"):
            DCUEDataset(trip.copy(), meta, neg_sampling="inverse")
        with pytest.raises(ValueError, match="neg_weights"):
            DCUEDataset(trip.copy(), meta, neg_sampling="weights")
        with pytest.raises(ValueError, match="neg_weights"):
            DCUEDataset(trip.copy(), meta, neg_weights=np.ones(n, dtype=np.int64))
        with pytest.raises(ValueError, match="per item"):
            DCUEDataset(trip.copy(), meta, neg_sampling="weights", neg_weights=np.ones(n + 1, np.int64)).negative_weights()
        with pytest.raises(ValueError, match="negative"):
            DCUEDataset(trip.copy(), meta, neg_sampling="weights", neg_weights=-np.ones(n, np.int64)).negative_weights()
        with pytest.raises(ValueError, match="2\\^32"):
            DCUEDataset(trip.copy(), meta, neg_sampling="weights",
                        neg_weights=np.full(n, 2 ** 31, np.int64)).negative_weights()
        with pytest.raises(ValueError, match="alpha"):
            DCUEDataset(trip.copy(), meta, neg_sampling="popularity", neg_alpha=-1.0).negative_weights()
    finally:
        np.random.set_state(state)


def test_train_dcue_options():
    import train_dcue
    a = train_dcue.parse(["--synthetic"])
    assert a.neg_sampling == "uniform" and a.neg_alpha == 0.75
    a = train_dcue.parse(["--synthetic", "--neg-sampling", "popularity", "--neg-alpha", "0.5"])
    assert a.neg_sampling == "popularity" and a.neg_alpha == 0.5
    for bad in (["--neg-sampling", "weights"], ["--neg-alpha", "-1"]):
        with pytest.raises(SystemExit):
            train_dcue.parse(["--synthetic"] + bad)
