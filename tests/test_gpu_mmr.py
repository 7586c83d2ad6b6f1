"""Diversity-aware serving on the GPU (include/dcue.h dcue_list_mmr / dcue_list_ild / dcue_list_ild_mean):
MMR re-ranking bit for bit against the fp64 reference where every similarity and every f is exactly
representable, within the derived tolerance on Gaussian factors (tests/mmr_reference.py
check_greedy_tolerant, at most 1 % of a case's steps off the fp64 strict argmax), short, degenerate and
flagged lists, independence of batching, ILD and its mean, and the trainer / WRMF surface."""
import functools
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import mmr_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RELS = {R.REL_RAW: "raw", R.REL_MINMAX: "minmax"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _div():
    from dcrecommend.nn import rank
    return rank.Diversify(DEV)


def _mmr(lists, rels, counts, feat, k_out, lam, rel_mode):
    out = _div().mmr_raw(_dev(lists.astype(np.int32)), _dev(rels.astype(np.float32)), _dev(counts.astype(np.int32)),
                         _dev(feat), k_out, lam, RELS[rel_mode])
    return [t.cpu().numpy() for t in out]


def _ref_mmr(lists, rels, counts, feat, k_out, lam, rel_mode):
    rows = [R.mmr(lists[i], rels[i], counts[i], feat, k_out, lam, rel_mode) for i in range(len(lists))]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32),
            np.array([r[3] for r in rows], np.int32))


def _same_bits(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[1].view(np.uint32), want[1].astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------------------- exact cases
def _exact_feat(rs, n_cand, d):
    """Rows in {0, +-1} with exactly 4 or 16 non-zeros: norms 2 or 4, every cosine a multiple of 1/16."""
    feat = np.zeros((n_cand, d), np.float32)
    for r in range(n_cand):
        nnz = 16 if d >= 16 and rs.rand() < 0.5 else 4
        feat[r, rs.choice(d, nnz, replace=False)] = rs.choice([-1.0, 1.0], nnz)
    return feat


def _exact_case(P, d, n=5, n_cand=300, seed=0):
    """Lists of distinct candidates with dyadic relevances in [0, 2], descending with many ties, the
    first 2 and the last 0 (min-max scaling divides by 2: exact)."""
    rs = np.random.RandomState(1000 * P + d + seed)
    feat = _exact_feat(rs, n_cand, d)
    lists = np.stack([rs.choice(n_cand, P, replace=False) for _ in range(n)]).astype(np.int32)
    rels = np.sort(rs.randint(0, 17, (n, P)) / 8.0, axis=1)[:, ::-1].astype(np.float32)
    rels[:, 0], rels[:, -1] = 2.0, (0.0 if P > 1 else 2.0)
    return feat, lists, np.ascontiguousarray(rels)


@pytest.mark.parametrize("d", [4, 16, 17, 128, 129, 256])
@pytest.mark.parametrize("P", [1, 2, 16, 17, 63, 64, 65, 128])
def test_exact_cases_match_the_reference_bit_for_bit(P, d):
    feat, lists, rels = _exact_case(P, d)
    full = np.full(len(lists), P, np.int32)
    mixed = np.array([P, P, max(P - 1, 0), P // 2, P + 5], np.int32)  # (P + 5: clamped to the pool)
    for k_out in sorted({1, P}):
        for rel_mode, counts in ((R.REL_RAW, full), (R.REL_RAW, mixed), (R.REL_MINMAX, full)):
            got = _mmr(lists, rels, counts, feat, k_out, 0.5, rel_mode)
            _same_bits(got, _ref_mmr(lists, rels, counts, feat, k_out, 0.5, rel_mode))


# ------------------------------------------------------------------------------- Gaussian cases
@functools.lru_cache(maxsize=None)
def _gaussian(d, score, n=64, n_cand=2000, P=128):
    """(feat, lists, rels, counts) of a real dcue_topk (cosine) / dcue_topk_scored (dot) call at k = P."""
    from dcrecommend.nn import rank
    rs = np.random.RandomState(77 + d)
    feat = rs.randn(n_cand, d).astype(np.float32)
    q = rs.randn(n, d).astype(np.float32)
    tk = rank.TopK(None, None, None, DEV, n_cand=n_cand, score=score)
    idx, sc, count, flags = tk.topk_raw(_dev(q), _dev(feat), np.arange(n), P)
    assert not flags.cpu().numpy().any()
    return feat, idx.cpu().numpy(), sc.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("rel_mode", [R.REL_RAW, R.REL_MINMAX])
@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("k_out", [10, 128])
@pytest.mark.parametrize("d", [16, 100, 128, 256])
def test_gaussian_cases_within_tolerance(d, k_out, lam, rel_mode):
    feat, lists, rels, counts = _gaussian(d, "cosine" if rel_mode == R.REL_RAW else "dot")
    assert np.all(counts == 128)
    idx, score, count, flags = _mmr(lists, rels, counts, feat, k_out, lam, rel_mode)
    assert not flags.any()
    steps = differ = 0
    for i in range(len(lists)):
        s, df = R.check_greedy_tolerant(idx[i], score[i], count[i], lists[i], rels[i], counts[i], feat, k_out, lam,
                                        rel_mode)
        steps, differ = steps + s, differ + df
    print("d=%d k_out=%d lam=%.1f rel=%s: %d of %d steps differ from the fp64 strict argmax"
          % (d, k_out, lam, RELS[rel_mode], differ, steps))
    assert steps == len(lists) * k_out and differ <= 0.01 * steps


@pytest.mark.parametrize("rel_mode", [R.REL_RAW, R.REL_MINMAX])
def test_one_dimensional_factors_all_ties(rel_mode):
    """d = 1: every similarity is +-1, so f ties everywhere (the tolerant check, without the cap)."""
    feat, lists, rels, counts = _gaussian(1, "cosine" if rel_mode == R.REL_RAW else "dot", n=8)
    for lam in (0.3, 0.7):
        idx, score, count, flags = _mmr(lists, rels, counts, feat, 128, lam, rel_mode)
        assert not flags.any()
        for i in range(len(lists)):
            R.check_greedy_tolerant(idx[i], score[i], count[i], lists[i], rels[i], counts[i], feat, 128, lam, rel_mode)


@pytest.mark.parametrize("rel_mode", [R.REL_RAW, R.REL_MINMAX])
def test_identities(rel_mode):
    feat, lists, rels, counts = _gaussian(100, "cosine" if rel_mode == R.REL_RAW else "dot")
    for k_out in (1, 10, 128):
        idx, score, count, flags = _mmr(lists, rels, counts, feat, k_out, 1.0, rel_mode)  # lambda = 1: the pool
        assert np.array_equal(idx, lists[:, :k_out]) and np.all(count == k_out) and not flags.any()
        assert np.array_equal(score.view(np.uint32), rels[:, :k_out].view(np.uint32))
    idx, score, _, _ = _mmr(lists, rels, counts, feat, 10, 0.0, rel_mode)  # lambda = 0: all f tie at 0 first
    assert np.array_equal(idx[:, 0], lists[:, 0]) and np.array_equal(score[:, 0], rels[:, 0])
    neg = -np.abs(rels) - 1  # negative relevances: lam * r' is -0, which must tie with +0
    idx, _, _, _ = _mmr(lists, np.sort(neg, axis=1)[:, ::-1].copy(), counts, feat, 3, 0.0, R.REL_RAW)
    assert np.array_equal(idx[:, 0], lists[:, 0])


# ------------------------------------------------------------------------------- short, degenerate, flagged
def test_short_and_degenerate_lists():
    P, d = 17, 16
    feat, lists, rels = _exact_case(P, d, n=8)
    feat[5] = 0.0  # a zero row: similarity 0 to everything
    lists[4, 3], lists[5, 0] = 5, 5
    lists[6, 9], rels[6, 9] = lists[6, 2], rels[6, 2]  # an index named twice: two entries, similarity 1
    lists[7, :] = lists[7, 0]  # ... and a pool of one index only
    counts = np.array([0, 1, 2, P - 1, P, P, P, P], np.int32)
    poisoned = lists.copy()
    for i, c in enumerate(counts):  # the tail past count is never read
        junk = np.array([-1, 2 ** 31 - 1, -7, len(feat), -2 ** 31], np.int64)
        poisoned[i, c:] = np.resize(junk, P - c).astype(np.int32)
    for k_out in (1, 5, P):
        want = _ref_mmr(lists, rels, counts, feat, k_out, 0.5, R.REL_RAW)
        assert want[2].tolist() == [min(k_out, c) for c in counts] and not want[3].any()
        _same_bits(_mmr(poisoned, rels, counts, feat, k_out, 0.5, R.REL_RAW), want)
    got = _mmr(poisoned, rels, counts, feat, P, 0.5, R.REL_RAW)
    assert sorted(got[0][6].tolist()).count(int(lists[6, 2])) == 2 and np.all(got[0][7] == lists[7, 0])


def test_flagged_lists_come_back_empty_and_neighbours_are_untouched():
    P, d, k_out = 33, 17, 20
    feat, lists, rels = _exact_case(P, d, n=9)
    counts = np.full(9, P, np.int32)
    clean = _mmr(lists, rels, counts, feat, k_out, 0.5, R.REL_RAW)
    assert not clean[3].any() and np.all(clean[2] == k_out)
    bad_lists, bad_rels, bad_feat = lists.copy(), rels.copy(), feat.copy()
    bad_lists[1, 7] = len(feat)  # one past the table
    bad_lists[3, 0] = -1
    bad_lists[4, P - 1] = 2 ** 31 - 1
    bad_rels[5, 2] = np.nan
    bad_rels[6, 30] = -np.inf
    nan_row = int(np.setdiff1d(lists[7], np.delete(lists, 7, axis=0))[0])
    bad_feat[nan_row, d - 1] = np.nan  # a row only list 7 names
    got = _mmr(bad_lists, bad_rels, counts, bad_feat, k_out, 0.5, R.REL_RAW)
    want_flags = [0, 2, 0, 2, 2, 4, 4, 4, 0]
    assert got[3].tolist() == want_flags
    _same_bits(got, _ref_mmr(bad_lists, bad_rels, counts, bad_feat, k_out, 0.5, R.REL_RAW))
    for i, f in enumerate(want_flags):
        if f:
            assert got[2][i] == 0 and np.all(got[0][i] == -1) and np.all(got[1][i] == -np.inf)
        else:
            assert all(np.array_equal(got[j][i], clean[j][i]) for j in range(4))
    # an out-of-range entry past count is not an error
    counts[1] = 7
    got = _mmr(bad_lists, bad_rels, counts, bad_feat, k_out, 0.5, R.REL_RAW)
    assert got[3][1] == 0 and got[2][1] == 7
    # ILD flags the same lists
    v, flags = [t.cpu().numpy() for t in _div().ild_raw(_dev(bad_lists), _dev(counts), _dev(bad_feat), (2, 10))]
    assert flags.tolist() == [0, 0, 0, 2, 2, 0, 0, 4, 0] and np.all(v[[3, 4, 7]] == 0)


# ------------------------------------------------------------------------------- batching
def test_lists_do_not_depend_on_batching():
    feat, lists, rels, counts = _gaussian(100, "dot")
    lists, rels, counts = lists[:50], rels[:50], counts[:50]
    whole = _mmr(lists, rels, counts, feat, 40, 0.7, R.REL_MINMAX)
    ild_whole = [t.cpu().numpy() for t in _div().ild_raw(_dev(lists), _dev(counts), _dev(feat), (2, 10, 128))]
    for step in (1, 7, 50):
        parts = [_mmr(lists[s:s + step], rels[s:s + step], counts[s:s + step], feat, 40, 0.7, R.REL_MINMAX)
                 for s in range(0, 50, step)]
        _same_bits([np.concatenate([p[j] for p in parts]) for j in range(4)], whole)
        ild = [[t.cpu().numpy() for t in _div().ild_raw(_dev(lists[s:s + step]), _dev(counts[s:s + step]), _dev(feat),
                                                        (2, 10, 128))] for s in range(0, 50, step)]
        assert np.array_equal(np.concatenate([p[0] for p in ild]), ild_whole[0])
        assert np.array_equal(np.concatenate([p[1] for p in ild]), ild_whole[1])


@pytest.mark.parametrize("score", ["cosine", "dot"])
def test_topk_with_diversity_does_not_depend_on_query_batch(score):
    from dcrecommend.nn import rank
    rs = np.random.RandomState(5)
    n_cand, d, n = 1500, 100, 50
    feat, q = rs.randn(n_cand, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    tk = rank.TopK(None, None, None, DEV, n_cand=n_cand, score=score)
    ref = tk.topk(_dev(q), _dev(feat), np.arange(n), 20, diversity=0.7)
    for qb in (1, 16, 4096):
        got = tk.topk(_dev(q), _dev(feat), np.arange(n), 20, query_batch=qb, diversity=0.7)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    # the documented route: the pool's top 80 (min(128, 4 k)), re-ranked with the score's default scaling
    idx, sc, count, _ = tk.topk_raw(_dev(q), _dev(feat), np.arange(n), 80)
    want = _div().mmr_raw(idx, sc, count, _dev(feat), 20, 0.7, "raw" if score == "cosine" else "minmax")
    assert np.array_equal(want[0].cpu().numpy(), ref[0]) and np.array_equal(want[1].cpu().numpy(), ref[1])
    plain = tk.topk(_dev(q), _dev(feat), np.arange(n), 20)
    for lam in (None, 1.0):  # off, and lambda = 1: the plain ranking's bits
        got = tk.topk(_dev(q), _dev(feat), np.arange(n), 20, diversity=lam)
        assert all(np.array_equal(a, b) for a, b in zip(got, plain))


# ------------------------------------------------------------------------------- ILD
@pytest.mark.parametrize("d", [16, 100, 256])
def test_ild_matches_the_reference(d):
    feat, lists, rels, counts = _gaussian(d, "cosine")
    counts = counts.copy()
    counts[:6] = [0, 1, 2, 9, 10, 127]
    ks = (1, 2, 10, 128)
    v, flags = [t.cpu().numpy() for t in _div().ild_raw(_dev(lists), _dev(counts), _dev(feat), ks)]
    for i in range(len(lists)):
        want, wf = R.ild(lists[i], counts[i], feat, ks)
        assert flags[i] == wf == R.FLAG_NO_PAIR and v[i, 0] == 0  # K = 1: no pair at any list
        assert np.abs(v[i] - want).max() <= R.tol_sim(d), (i, v[i], want)
    assert np.all(v[0] == 0) and np.all(v[1] == 0) and v[2, 1] > 0 and v[2, 1] == v[2, 2] == v[2, 3]
    v2, flags2 = [t.cpu().numpy() for t in _div().ild_raw(_dev(lists), _dev(counts), _dev(feat), (2, 10, 128))]
    assert flags2.tolist() == [1, 1] + [0] * (len(lists) - 2) and np.array_equal(v2, v[:, 1:])


def _fsum_mean(v, flags):
    keep = flags == 0
    n = int(keep.sum())
    return np.array([math.fsum(v[keep, j]) / n if n else 0.0 for j in range(v.shape[1])]), n


def test_ild_mean_of_real_lists():
    feat, lists, rels, counts = _gaussian(100, "cosine")
    lists, counts = lists[:50], counts[:50].copy()
    counts[[3, 17]] = [1, 0]
    ks = (2, 10, 128)
    v, flags = _div().ild_raw(_dev(lists), _dev(counts), _dev(feat), ks)
    mean, n = [t.cpu().numpy() for t in _div().ild_mean_raw(v, flags)]
    want, wn = _fsum_mean(v.cpu().numpy(), flags.cpu().numpy())
    assert n[0] == wn == 48 and np.abs(mean - want).max() <= 1e-15 * np.abs(want).max()
    for step in (1, 7):  # however `ild` was filled
        parts = [_div().ild_raw(_dev(lists[s:s + step]), _dev(counts[s:s + step]), _dev(feat), ks)
                 for s in range(0, 50, step)]
        m2, n2 = _div().ild_mean_raw(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
        assert np.array_equal(m2.cpu().numpy(), mean) and n2.cpu().numpy()[0] == 48


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 1025, 3000])
def test_ild_mean_reduction(n, m):
    """The reduction alone on synthetic values: any order of n non-negative fp64 additions is within
    n 2^-53 relative of the exact sum."""
    rs = np.random.RandomState(n + m)
    v = rs.rand(n, m) * 2
    flags = (rs.rand(n) < 0.2).astype(np.int32) * rs.randint(1, 8, n).astype(np.int32)
    mean, cnt = [t.cpu().numpy() for t in _div().ild_mean_raw(_dev(v), _dev(flags))]
    want, wn = _fsum_mean(v, flags)
    assert cnt[0] == wn and np.all(np.abs(mean - want) <= max(n, 1) * 2.0 ** -53 * np.abs(want))
    if n:
        again = _div().ild_mean_raw(_dev(v), _dev(flags))[0].cpu().numpy()
        assert np.array_equal(again, mean)


# ------------------------------------------------------------------------------- trainer and WRMF
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
    """The tiny trainer of the top-K tests: golden weights, factors computed on the GPU."""
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
    return g, tr, train, val


def _clustered(rs, n_items, d, per_cluster):
    """Tight clusters of per_cluster items around random unit centres: the plain ranking fills a list
    from one cluster, so its intra-list diversity is near 0."""
    centres = rs.randn((n_items + per_cluster - 1) // per_cluster, d)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    return (np.repeat(centres, per_cluster, axis=0)[:n_items] + 0.01 * rs.randn(n_items, d)).astype(np.float32)


def test_dcue_recommend_and_evaluate_topk(trained):
    g, tr, train, val = trained
    users = list(g["val_users"][:6])
    plain = tr.recommend(users, k=5, dataset=val, as_ids=False)
    same = tr.recommend(users, k=5, dataset=val, as_ids=False, diversity=None)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))
    assert tr.recommend(users, k=5, dataset=val) == tr.recommend(users, k=5, dataset=val, diversity=None, pool=None)
    ks = (2, 5)
    old = tr.evaluate_topk(ks=ks)
    new = tr.evaluate_topk(ks=ks, ild=True)
    assert set(new) == set(old) | {"ild@2", "ild@5", "n_ild"} and all(new[k] == old[k] for k in old)
    assert new["n_ild"] == old["n_users"] and 0.0 <= new["ild@2"] <= 2.0 and 0.0 <= new["ild@5"] <= 2.0
    assert tr.evaluate_topk(ks=ks, diversity=None) == old
    # ild@K against the reference on the lists recommend() returns
    all_users = [train.userindex2userid[int(r)] for r in tr._topk_metrics(None)[1]]
    idx, _, count = tr.recommend(all_users, k=5, exclude_seen=False, as_ids=False)
    feat = tr._item_feat_by_index().cpu().numpy()
    want = np.mean([R.ild(idx[i], count[i], feat, ks)[0] for i in range(len(idx))], axis=0)
    tol = R.tol_sim(feat.shape[1])
    assert abs(new["ild@2"] - want[0]) <= tol and abs(new["ild@5"] - want[1]) <= tol
    # the diversified lists are a re-ranking of the pool, in MMR's order, on the pairs interface too
    div = tr.recommend(users, k=5, dataset=None, as_ids=False, diversity=0.5, pool=12)
    pool = tr.recommend(users, k=12, dataset=None, as_ids=False)
    for i in range(len(users)):
        want_i = R.mmr(pool[0][i].astype(np.int32), pool[1][i], pool[2][i], feat, 5, 0.5, R.REL_RAW)
        R.check_greedy_tolerant(div[0][i], div[1][i], div[2][i], pool[0][i], pool[1][i], pool[2][i], feat, 5, 0.5,
                                R.REL_RAW)
        assert want_i[2] == div[2][i]
    pairs = tr.recommend(users, k=5, diversity=0.5, pool=12)
    names = train.itemindex2songid
    want_names = [[names[int(j)] for j in div[0][i, :div[2][i]]] for i in range(len(users))]
    assert [[s for s, _ in lst] for lst in pairs] == want_names
    with pytest.raises(ValueError, match=r"k\.\.128"):
        tr.recommend(users, k=5, diversity=0.5, pool=4)
    with pytest.raises(ValueError, match="diversity"):
        tr.recommend(users, k=5, pool=8)
    # tight clusters: MMR raises the intra-list diversity by construction
    saved = tr.item_factors, tr.user_factors
    rs = np.random.RandomState(9)
    try:
        tr.item_factors = _dev(_clustered(rs, saved[0].shape[0], saved[0].shape[1], 4))
        tr.user_factors = _dev(rs.randn(*saved[1].shape).astype(np.float32))
        base = tr.evaluate_topk(ks=ks, ild=True)
        mmr = tr.evaluate_topk(ks=ks, ild=True, diversity=0.5)
        print("clustered DCUE factors: ild", [base["ild@%d" % k] for k in ks], "->", [mmr["ild@%d" % k] for k in ks])
        assert all(mmr["ild@%d" % k] >= base["ild@%d" % k] for k in ks) and mmr["ild@5"] > base["ild@5"]
        assert set(mmr) == set(new) and mmr["n_ild"] == base["n_ild"]
    finally:
        tr.item_factors, tr.user_factors = saved


def test_dcue_recommend_for_with_diversity(trained):
    g, tr, train, val = trained
    songs = [s for s in g["meta_songs"] if s in train.item_index]
    histories = [songs[:5], songs[7:10]]
    plain = tr.recommend_for(histories, k=4, as_ids=False, steps=3)
    assert all(np.array_equal(a, b) for a, b in zip(plain, tr.recommend_for(histories, k=4, as_ids=False, steps=3,
                                                                            diversity=None)))
    assert all(np.array_equal(a, b) for a, b in zip(plain, tr.recommend_for(histories, k=4, as_ids=False, steps=3,
                                                                            diversity=1.0)))
    div = tr.recommend_for(histories, k=4, as_ids=False, steps=3, diversity=0.3, pool=10)
    pool = tr.recommend_for(histories, k=10, as_ids=False, steps=3)
    feat = tr._item_feat_by_index().cpu().numpy()
    for i in range(2):
        R.check_greedy_tolerant(div[0][i], div[1][i], div[2][i], pool[0][i], pool[1][i], pool[2][i], feat, 4, 0.3,
                                R.REL_RAW)


def _wrmf(n_users, n_items, d, seed):
    """A WRMF with clustered item factors in place (no fit) and random interactions."""
    from dcrecommend.dcbr import WRMF, device_csr
    rs = np.random.RandomState(seed)
    m = WRMF(factors=d, regularization=0.1, alpha=2.0, iterations=0, device=DEV)
    rows = np.repeat(np.arange(n_users), 3)
    cols = rs.randint(0, n_items, len(rows))
    r, c = torch.as_tensor(rows, device=DEV), torch.as_tensor(cols, device=DEV)
    m.by_user = device_csr(r, c, None, n_users)
    m.by_item = device_csr(c, r, None, n_items)
    m.init_factors(n_users, n_items)
    m.item_factors.copy_(_dev(_clustered(rs, n_items, d, 8) * rs.uniform(0.5, 3.0, (n_items, 1)).astype(np.float32)))
    m.user_factors.copy_(_dev(rs.randn(n_users, d).astype(np.float32)))
    truth = [np.unique(rs.randint(0, n_items, 4)) for _ in range(n_users)]
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in truth])]).astype(np.int64)
    return m, tptr, np.concatenate(truth).astype(np.int32)


def test_wrmf_recommend_and_evaluate_topk():
    m, tptr, tidx = _wrmf(40, 400, 24, seed=3)
    users = np.arange(40)
    plain = m.recommend(users, 10)
    assert all(np.array_equal(a, b) for a, b in zip(plain, m.recommend(users, 10, diversity=None, pool=None)))
    assert all(np.array_equal(a, b) for a, b in zip(plain, m.recommend(users, 10, diversity=1.0)))
    ks = (2, 10)
    old = m.evaluate_topk(tptr, tidx, ks=ks)
    new = m.evaluate_topk(tptr, tidx, ks=ks, ild=True)
    assert set(new) == set(old) | {"ild@2", "ild@10", "n_ild"} and all(new[k] == old[k] for k in old)
    assert m.evaluate_topk(tptr, tidx, ks=ks, diversity=None, pool=None, ild=False) == old
    # dot scores, min-max relevance: the diversified list against the reference under its own prefix
    Y = m.item_factors.cpu().numpy()
    div = m.recommend(users, 10, diversity=0.5)
    pool = m.recommend(users, 40)
    for i in range(len(users)):
        R.check_greedy_tolerant(div[0][i], div[1][i], div[2][i], pool[0][i], pool[1][i], pool[2][i], Y, 10, 0.5,
                                R.REL_MINMAX)
    mmr = m.evaluate_topk(tptr, tidx, ks=ks, ild=True, diversity=0.5)
    print("clustered WRMF factors: ild", [new["ild@%d" % k] for k in ks], "->", [mmr["ild@%d" % k] for k in ks])
    assert all(mmr["ild@%d" % k] >= new["ild@%d" % k] for k in ks) and mmr["ild@10"] > new["ild@10"]
    hist = [[1, 2, 3], [10, 11]]
    got = m.recommend_for(hist, 5, diversity=0.5, pool=20)
    base = m.recommend_for(hist, 20)
    for i in range(2):
        R.check_greedy_tolerant(got[0][i], got[1][i], got[2][i], base[0][i], base[1][i], base[2][i], Y, 5, 0.5,
                                R.REL_MINMAX)


def test_train_dcue_driver_with_diversity(tmp_path):
    import json
    import train_dcue
    recs, out = tmp_path / "r.csv", tmp_path / "m.json"
    train_dcue.main(["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80", "--synthetic-pairs", "300",
                     "--feature-dim", "32", "--conv-hidden", "32", "--batch-size", "8", "--neg-batch-size", "3",
                     "--num-epochs", "1", "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path / "ck"),
                     "--recommend-k", "5",
                     "--recommend-out", str(recs), "--recommend-diversity", "0.7", "--recommend-pool", "12",
                     "--eval-k", "2,5", "--eval-out", str(out), "--eval-ild", "--eval-diversity", "0.7"])
    res = json.loads(out.read_text())
    for split in ("val", "test"):
        assert {"ild@2", "ild@5", "n_ild", "ndcg@5", "n_users"} <= set(res[split])
        assert 0.0 <= res[split]["ild@5"] <= 2.0
    df = pd.read_csv(recs)
    assert set(df.columns) == {"user_id", "rank", "song_id", "score"} and df["rank"].max() <= 5 and len(df) > 0
