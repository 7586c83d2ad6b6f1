"""GPU tests of the fused top-K recommendation (dcue_topk, rank.TopK, DCUE.recommend /
similar_songs, train_dcue.py --recommend-k) against the numpy reference in topk_reference.py.

Exact cases use lattice factors (rows of 16 entries +-1: norm exactly 4, every cosine a multiple of
1/16, exact in fp32 in any summation order), so indices, counts and score bits must equal the fp64
reference's, tie order included. Gaussian cases are held to tol = (dp + 8) 2^-24: the fp32
accumulation bound of a dp-term dot product of unit vectors (dp 2^-24) plus a few ulps for the two
normalisations; near-ties within 2 tol of the k-th best score may fall either way, nothing else.
"""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import topk_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lattice(rs, n, d):
    x = np.zeros((n, d), np.float32)
    for r in range(n):
        x[r, rs.choice(d, 16, replace=False)] = rs.choice(np.array([-1.0, 1.0], np.float32), 16)
    return x


@functools.lru_cache(maxsize=None)
def _case(seed, n_rows, n_cand, d, n_queries, lattice, max_excl=150):
    """Factors with duplicated rows (exact ties) and zero rows, random exclusion rows of 0..max_excl
    sorted items, a random mask, queries with repeats, and the fp64 cosines of the queries."""
    rs = np.random.RandomState(seed)
    cand = _lattice(rs, n_cand, d) if lattice else rs.randn(n_cand, d).astype(np.float32)
    dup = rs.choice(n_cand, n_cand // 20, replace=False)
    cand[dup] = cand[rs.choice(n_cand, len(dup))]
    cand[rs.choice(n_cand, 3, replace=False)] = 0.0
    qf = _lattice(rs, n_rows, d) if lattice else rs.randn(n_rows, d).astype(np.float32)
    ptr, idx = [0], []
    for r in range(n_rows):
        n = rs.randint(0, max_excl + 1)
        idx.append(np.sort(rs.choice(n_cand, n, replace=False)))
        ptr.append(ptr[-1] + n)
    mask = (rs.rand(n_cand) < 0.8).astype(np.uint8)
    queries = rs.randint(0, n_rows, n_queries)
    c = dict(qf=qf, cand=cand, ptr=np.array(ptr, np.int64), idx=np.concatenate(idx).astype(np.int32), mask=mask,
             queries=queries)
    c["s64"] = T.cosines(qf, cand, queries)
    return c


def _run(c, k, query_batch=None, cand_split=0, excl=True, mask=True, raw=False):
    from dcrecommend.nn import rank
    tk = rank.TopK(c["ptr"] if excl else None, c["idx"] if excl else None, c["mask"] if mask else None, DEV,
                   n_cand=len(c["cand"]))
    fn = tk.topk_raw if raw else tk.topk
    return fn(torch.from_numpy(c["qf"]).to(DEV), torch.from_numpy(c["cand"]).to(DEV), c["queries"], k,
              query_batch=query_batch, cand_split=cand_split)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _assert_exact(got, c, k, excl=True, mask=True):
    want = T.topk(None, None, c["queries"], k, c["ptr"] if excl else None, c["idx"] if excl else None,
                  c["mask"] if mask else None, scores=c["s64"])
    idx, score, count = got
    assert idx.dtype == np.int64 and score.dtype == np.float32 and count.dtype == np.int32
    assert np.array_equal(count, want[2])
    assert np.array_equal(idx, want[0])
    assert np.array_equal(_bits(score), _bits(want[1] + 0.0))


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("d", [32, 100, 128, 256])
def test_lattice_exact(d, k):
    c = _case(5 + d, 130, 2500, d, 150, True)
    _assert_exact(_run(c, k), c, k)


@pytest.mark.parametrize("lattice,d,k", [(True, 100, 10), (False, 128, 50)])
def test_deterministic_across_tilings(lattice, d, k):
    """idx and the raw bits of score do not depend on cand_split or query_batch."""
    c = _case(5 + d, 130, 2500, d, 150, True) if lattice else _case(77, 130, 5003, d, 130, False)
    first = None
    for split in (1, 2, 5, 0):
        for qb in (16, 64, 1000):
            idx, score, count = _run(c, k, query_batch=qb, cand_split=split)
            if first is None:
                first = (idx, _bits(score), count)
                continue
            assert np.array_equal(idx, first[0]), (split, qb)
            assert np.array_equal(_bits(score), first[1]), (split, qb)
            assert np.array_equal(count, first[2]), (split, qb)
    if lattice:
        _assert_exact((first[0], first[1].view(np.float32), first[2]), c, k)


@pytest.mark.parametrize("d", [100, 128])
def test_gaussian_vs_fp64(d):
    k = 50
    c = _case(70 + d, 130, 5003, d, 130, False)
    idx, score, count = _run(c, k)
    tol = ((d + 15) // 16 * 16 + 8) * 2.0 ** -24
    for i, q in enumerate(c["queries"]):
        ok = T.eligible(c["s64"][i], int(q), c["ptr"], c["idx"], c["mask"])
        T.check_tolerant(idx[i], score[i], int(count[i]), c["s64"][i], ok, k, tol)


# ------------------------------------------------------------------------------------- edges
def test_fewer_candidates_than_k_pads():
    c = _case(1, 20, 70, 32, 25, True, max_excl=10)
    got = _run(c, 128)
    assert np.all(got[2] < 128) and np.all(got[0][:, 70:] == -1) and np.all(np.isneginf(got[1][:, 70:]))
    _assert_exact(got, c, 128)


def test_exactly_three_eligible():
    c = dict(_case(2, 20, 300, 32, 25, True, max_excl=10))
    keep = np.array([5, 64, 299])
    rows = [np.setdiff1d(np.arange(300), keep) if r == 7 else np.array([r], np.int64) for r in range(20)]
    c["ptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    c["idx"] = np.concatenate(rows).astype(np.int32)
    c["mask"] = np.ones(300, np.uint8)
    c["queries"] = np.array([7, 3, 7, 0])
    c["s64"] = T.cosines(c["qf"], c["cand"], c["queries"])
    got = _run(c, 10)
    assert got[2].tolist() == [3, 10, 3, 10] and sorted(got[0][0, :3].tolist()) == keep.tolist()
    _assert_exact(got, c, 10)


def test_exclusions_at_tile_edges():
    n = 200
    c = dict(_case(3, 20, n, 32, 25, True, max_excl=10))
    edge = np.array([63, 64, n - 1], np.int32)
    c["ptr"] = np.arange(21, dtype=np.int64) * 3
    c["idx"] = np.tile(edge, 20)
    c["mask"] = np.ones(n, np.uint8)
    for split in (0, 2):
        got = _run(c, 128, cand_split=split)
        assert not np.isin(got[0], edge).any() and np.all(got[2] == 128)
        _assert_exact(got, c, 128)


def test_mask_with_a_single_one():
    c = dict(_case(4, 20, 300, 32, 25, True, max_excl=10))
    c["mask"] = np.zeros(300, np.uint8)
    c["mask"][130] = 1
    got = _run(c, 10, excl=False)
    assert np.all(got[2] == 1) and np.all(got[0][:, 0] == 130) and np.all(got[0][:, 1:] == -1)
    _assert_exact(got, c, 10, excl=False)


def test_single_query():
    c = dict(_case(5, 130, 2500, 100, 150, True))
    c["queries"] = c["queries"][:1]
    c["s64"] = c["s64"][:1]
    _assert_exact(_run(c, 10), c, 10)


def test_null_mask_and_null_exclusion():
    c = _case(6, 130, 2500, 100, 150, True)
    _assert_exact(_run(c, 10, excl=False, mask=False), c, 10, excl=False, mask=False)
    _assert_exact(_run(c, 10, excl=True, mask=False), c, 10, excl=True, mask=False)


def test_shape_and_index_checks():
    from dcrecommend.nn import rank
    c = _case(6, 130, 2500, 100, 150, True)
    tk = rank.TopK(c["ptr"], c["idx"], c["mask"], DEV)
    qf, cand = torch.from_numpy(c["qf"]).to(DEV), torch.from_numpy(c["cand"]).to(DEV)
    with pytest.raises(ValueError):
        tk.topk(qf, cand[:100], [0], 10)
    with pytest.raises(ValueError):
        tk.topk(qf[:50], cand, [0], 10)
    with pytest.raises(IndexError):
        tk.topk(qf, cand, [130], 10)
    with pytest.raises(ValueError):
        tk.topk(qf, cand, [0], 129)


# ------------------------------------------------------------------------------------- non-finite
def test_nan_candidate_flags_the_queries_that_could_see_it():
    c = dict(_case(8, 40, 1500, 64, 60, False, max_excl=40))
    # a candidate that the first query's row excludes (and few others do), admitted by the mask
    first = c["queries"][0]
    bad = int(c["idx"][c["ptr"][first]])
    c["mask"] = c["mask"].copy()
    c["mask"][bad] = 1
    cand = c["cand"].copy()
    cand[bad] = np.nan
    c["cand"] = cand
    with pytest.raises(ValueError, match="Input contains NaN"):
        _run(c, 20)
    idx, score, count, flags = [t.cpu().numpy() for t in _run(c, 20, raw=True)]
    sees = np.array([bad not in c["idx"][c["ptr"][q]:c["ptr"][q + 1]] for q in c["queries"]])
    assert sees.any() and not sees.all()
    assert np.array_equal((flags & 2) != 0, sees)
    assert not (idx == bad).any()
    # the other candidates' lists are what they are without the NaN row
    s64 = c["s64"].copy()
    s64[:, bad] = np.nan
    tol = (64 + 8) * 2.0 ** -24
    for i, q in enumerate(c["queries"]):
        ok = T.eligible(s64[i], int(q), c["ptr"], c["idx"], c["mask"])
        T.check_tolerant(idx[i].astype(np.int64), score[i], int(count[i]), s64[i], ok, 20, tol)
    # a NaN candidate the mask drops is never scored for anyone
    c["mask"] = c["mask"].copy()
    c["mask"][bad] = 0
    assert not (_run(c, 20, raw=True)[3].cpu().numpy() & 2).any()


def test_nan_query_flags_only_itself():
    c = dict(_case(9, 40, 1500, 64, 60, False, max_excl=40))
    row = int(c["queries"][4])
    qf = c["qf"].copy()
    qf[row] = np.nan
    c["qf"] = qf
    with pytest.raises(ValueError, match="Input contains NaN"):
        _run(c, 20)
    idx, score, count, flags = [t.cpu().numpy() for t in _run(c, 20, raw=True)]
    hit = c["queries"] == row
    assert np.array_equal((flags & 2) != 0, hit)
    assert np.all(count[hit] == 0) and np.all(idx[hit] == -1) and np.all(count[~hit] == 20)


# ------------------------------------------------------------------------------------- trainer
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
        tr.recommend([g["val_users"][0]])
    tr._user_factors(items)
    tr._item_factors(items)
    with pytest.raises(RuntimeError, match="exclude_seen"):
        tr.recommend([g["val_users"][0]])  # no dataset given and none bound by fit()
    tr.train_data = train
    return g, tr, train, val, items


def _predict_rows(tr, u, val):
    """predict(u, val) as (scores over item indices (NaN where not listed), label-0 set, positives)."""
    sp, tp = tr.predict(u, val)
    ui = val.user_index[u]
    pos = [val.item_index[s] for s in val.triplets.loc[val.triplets['user_id'] == u, 'song_id']]
    inter = set(val.item_user.getcol(ui).nonzero()[0].tolist())
    rest = [i for i in val.split_items().tolist() if i not in inter]
    s = np.full(val.n_items, np.nan)
    s[np.array(pos + rest)] = np.array(sp, np.float64)
    ok = np.zeros(val.n_items, bool)
    ok[rest] = True
    return s, ok, pos


def test_recommend_matches_predict(trained):
    g, tr, train, val, items = trained
    d = int(g["d"])
    tol = ((d + 15) // 16 * 16 + 8) * 2.0 ** -24
    for u in list(g["val_users"][:3]):
        s, ok, pos = _predict_rows(tr, u, val)
        idx, score, count = tr.recommend([u], k=10, dataset=val, as_ids=False)
        T.check_tolerant(idx[0], score[0], int(count[0]), s, ok, 10, tol)
        pairs = tr.recommend([u], k=10, dataset=val)[0]
        assert [p[0] for p in pairs] == [val.itemindex2songid[int(i)] for i in idx[0, :count[0]]]
        assert [p[1] for p in pairs] == [float(x) for x in score[0, :count[0]]]
        # with the seen songs allowed, the user's best played val song is there when it beats the 10th
        idx2, score2, count2 = tr.recommend([u], k=10, dataset=val, exclude_seen=False, as_ids=False)
        best = max(pos, key=lambda i: s[i])
        if count2[0] < 10 or s[best] > float(score2[0, 9]) + 2 * tol:
            assert best in idx2[0].tolist()
    # no dataset: every song with audio, minus the seen ones
    idx, score, count = tr.recommend(list(g["val_users"][:3]), k=5, as_ids=False)
    ptr, seen = train.user_item_csr()
    for r, u in enumerate(g["val_users"][:3]):
        ui = train.user_index[u]
        assert not np.isin(idx[r, :count[r]], seen[ptr[ui]:ptr[ui + 1]]).any()
    with pytest.raises(KeyError):
        tr.recommend(["no such user"], k=10, dataset=val)


def test_similar_songs_excludes_the_query(trained):
    g, tr, train, val, items = trained
    songs = list(g["val_songs"][:5])
    for song, lst in zip(songs, tr.similar_songs(songs, k=10)):
        assert len(lst) == 10 and song not in [s for s, _ in lst]
        assert all(a[1] >= b[1] for a, b in zip(lst, lst[1:]))
    for song, lst in zip(songs, tr.similar_songs(songs, k=3, dataset=val)):
        assert song not in [s for s, _ in lst] and all(s in set(val.uniq_songs) for s, _ in lst)


def test_train_dcue_driver_writes_recommendations(tmp_path):
    import train_dcue
    out = tmp_path / "rec.csv"
    argv = ["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80", "--synthetic-pairs", "300",
            "--feature-dim", "32", "--conv-hidden", "32", "--batch-size", "8", "--neg-batch-size", "3",
            "--num-epochs", "1", "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path / "ck"),
            "--recommend-k", "5", "--recommend-out", str(out)]
    dcue = train_dcue.main(argv)
    rec = pd.read_csv(out)
    assert list(rec.columns) == ["user_id", "rank", "song_id", "score"]
    users = list(dcue.train_data.uniq_users)
    assert sorted(set(rec["user_id"])) == sorted(users)
    coo = dcue.train_data.item_user.tocoo()  # every split's interactions
    played = set((dcue.train_data.userindex2userid[c], dcue.train_data.itemindex2songid[r])
                 for r, c in zip(coo.row, coo.col))
    assert len(played) == 300
    for u, grp in rec.groupby("user_id"):
        assert grp["rank"].tolist() == [1, 2, 3, 4, 5]
        assert grp["score"].tolist() == sorted(grp["score"], reverse=True)
        assert len(set(grp["song_id"])) == 5
        assert not any((u, s) in played for s in grp["song_id"])
