"""End-to-end GPU tests of artist-aware serving on a tiny model whose factors are set directly: 120 songs
(so ONE dcue_topk call at k = 120 is a user's full ranking, in the library's own order), 9 artists of which
one owns 80 songs, three songs without an artist, 40 users. The oracle is that full ranking pushed through
group_reference.py's sequential cap. Every comparison is exact (indices with ==, scores by their bits)."""
import numpy as np
import pandas as pd
import pytest
import torch

import group_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SONGS, N_USERS, D, BIG = 120, 40, 16, 80


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _catalogue():
    """(songs, {song: artist}, played rows per user). Artist A0 owns the first 80 songs, A1..A8 share 37,
    the last 3 songs have no artist."""
    rs = np.random.RandomState(42)
    songs = ["S%03d" % i for i in range(N_SONGS)]
    amap = {s: "A0" for s in songs[:BIG]}
    for j, s in enumerate(songs[BIG:N_SONGS - 3]):
        amap[s] = "A%d" % (1 + j % 8)
    played = [sorted(set([songs[u], songs[u + N_USERS], songs[u + 2 * N_USERS]] + list(rs.choice(songs, 4))))
              for u in range(N_USERS)]
    return songs, amap, played


def _factors():
    """Gaussian user and item factors: by its size alone the big artist holds two thirds of every ranking,
    so at cap 2 a user's tenth survivor lies up to about 40 entries deep -- past a pool of 16 for most
    users, within four rounds of it for all."""
    rs = np.random.RandomState(7)
    return rs.randn(N_USERS, D).astype(np.float32), rs.randn(N_SONGS, D).astype(np.float32)


@pytest.fixture(scope="module")
def tiny():
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.nn.dcue import DCUE
    songs, amap, played = _catalogue()
    trip = pd.DataFrame([("U%02d" % u, s, 1.0) for u, row in enumerate(played) for s in row],
                        columns=["user_id", "song_id", "score"])
    meta = pd.DataFrame({"idx": np.arange(N_SONGS), "song_id": songs, "data_mel": ["none"] * N_SONGS})
    ds = DCUEDataset(trip, meta, split="all")
    assert ds.n_items == N_SONGS and ds.n_users == N_USERS
    users, items = _factors()
    tr = DCUE(feature_dim=D, device=DEV)
    tr.user_factors = torch.from_numpy(users).to(DEV)
    tr.item_factors = torch.from_numpy(items).to(DEV)
    tr._item_meta = np.arange(N_SONGS)
    tr.train_data = ds
    tr.set_artists(amap)
    group_of, names = tr._artist_groups(None)
    assert names == ["A%d" % a for a in range(9)] and (group_of == 0).sum() == BIG and (group_of < 0).sum() == 3
    uids = ["U%02d" % u for u in range(N_USERS)]
    # the full rankings, seen songs excluded: what every capped list must be a cap of
    full = tr._topk("user", None, True).topk(tr.user_factors, tr._item_feat_by_index(), np.arange(N_USERS), N_SONGS)
    return dict(tr=tr, ds=ds, uids=uids, group_of=group_of, names=names, full=full, played=played, songs=songs)


def _ranking(full, u):
    idx, score, count = full
    return idx[u, :count[u]], score[u, :count[u]]


def _assert_lists(got, want_idx, want_score):
    idx, score, count = got
    for r in range(len(count)):
        assert idx[r, :count[r]].tolist() == list(want_idx[r]), r
        assert np.array_equal(_bits(score[r, :count[r]]), _bits(want_score[r])), r
        assert (idx[r, count[r]:] == -1).all() and np.isneginf(score[r, count[r]:]).all()


def test_capped_recommend_equals_the_cap_of_the_full_ranking(tiny):
    tr, g = tiny["tr"], tiny["group_of"]
    want = [R.cap_full_ranking(*_ranking(tiny["full"], u), g, 2, 10) for u in range(N_USERS)]
    got = tr.recommend(tiny["uids"], 10, max_per_artist=2, pool=16, as_ids=False)
    tk = tr._topk("user", None, True)
    assert tk.cap_rounds_used >= 2  # the pool of 16 did not hold 10 survivors for everybody: deepening ran
    assert (got[2] == 10).all()
    _assert_lists(got, [w[0] for w in want], [w[1] for w in want])
    flags = tk.topk_raw(tr.user_factors, tr._item_feat_by_index(), np.arange(N_USERS), 10, pool=16, group_of=g,
                        max_per_group=2)[3].cpu().numpy()
    assert not flags.any()
    pairs = tr.recommend(tiny["uids"][:3], 10, max_per_artist=2, pool=16)
    assert [[s for s, _ in row] for row in pairs] == [[tiny["songs"][i] for i in w[0]] for w in want[:3]]


def test_one_round_returns_the_pool_only_result_and_says_short(tiny):
    from dcrecommend import _native as nat
    tr, g = tiny["tr"], tiny["group_of"]
    want = []
    for u in range(N_USERS):
        idx, score = _ranking(tiny["full"], u)
        want.append(R.cap_full_ranking(idx[:16], score[:16], g, 2, 10))
    short = np.array([len(w[0]) < 10 for w in want])
    assert short.any() and not short.all()
    got = tr.recommend(tiny["uids"], 10, max_per_artist=2, pool=16, cap_rounds=1, as_ids=False)
    _assert_lists(got, [w[0] for w in want], [w[1] for w in want])
    tk = tr._topk("user", None, True)
    assert tk.cap_rounds_used == 1
    flags = tk.topk_raw(tr.user_factors, tr._item_feat_by_index(), np.arange(N_USERS), 10, pool=16, group_of=g,
                        max_per_group=2, cap_rounds=1)[3].cpu().numpy()
    assert np.array_equal((flags & nat.GROUP_FLAG_SHORT) != 0, short) and not (flags & ~nat.GROUP_FLAG_SHORT).any()


def test_recommend_artists_is_first_appearance_order(tiny):
    tr, g, names = tiny["tr"], tiny["group_of"], tiny["names"]
    got = tr.recommend_artists(tiny["uids"], 5)
    for u in range(N_USERS):
        want, seen = [], set()
        for i, s in zip(*_ranking(tiny["full"], u)):
            if g[i] >= 0 and g[i] not in seen:
                seen.add(g[i])
                want.append((names[g[i]], tiny["songs"][i], s))
        assert [(a, s) for a, s, _ in got[u]] == [(a, s) for a, s, _ in want[:5]], u
        assert np.array_equal(_bits([x for _, _, x in got[u]]), _bits([x for _, _, x in want[:5]]))


def test_similar_songs_by_other_artists(tiny):
    tr, g = tiny["tr"], tiny["group_of"]
    feat = tr._item_feat_by_index()
    rows = np.array([0, 5, 79, 80, 95, 117, 119])  # big artist, small artists, songs without an artist
    full = tr._topk("song", None, True).topk(feat, feat, rows, N_SONGS - 1)
    got = tr.similar_songs([tiny["songs"][r] for r in rows], 12, other_artists=True)
    for n, r in enumerate(rows):
        idx, score = _ranking(full, n)
        keep = (g[idx] != g[r]) | (g[r] < 0)
        assert [s for s, _ in got[n]] == [tiny["songs"][i] for i in idx[keep][:12]], r
        assert np.array_equal(_bits([x for _, x in got[n]]), _bits(score[keep][:12]))
        assert g[r] < 0 or all(g[tiny["songs"].index(s)] != g[r] for s, _ in got[n])
    capped = tr.similar_songs([tiny["songs"][0]], 8, max_per_artist=1, pool=32)
    want = R.cap_full_ranking(*_ranking(full, 0), g, 1, 8)
    assert [s for s, _ in capped[0]] == [tiny["songs"][i] for i in want[0]]


def test_new_artists_drops_every_song_of_a_played_artist(tiny):
    tr, g = tiny["tr"], tiny["group_of"]
    nosee = tr._topk("user", None, False).topk(tr.user_factors, tr._item_feat_by_index(), np.arange(N_USERS), N_SONGS)
    got = tr.recommend(tiny["uids"], 10, new_artists=True, as_ids=False)
    some = False
    for u in range(N_USERS):
        mine = np.array([tiny["songs"].index(s) for s in tiny["played"][u]])
        heard = set(g[mine][g[mine] >= 0].tolist())
        idx, score = _ranking(nosee, u)
        keep = np.array([g[i] not in heard and i not in mine for i in idx])
        assert got[0][u, :got[2][u]].tolist() == idx[keep][:10].tolist(), u
        assert np.array_equal(_bits(got[1][u, :got[2][u]]), _bits(score[keep][:10]))
        some |= bool(got[2][u])
    assert some


def test_diversity_picks_from_the_capped_pool(tiny):
    from dcrecommend.nn import rank
    tr, g = tiny["tr"], tiny["group_of"]
    got = tr.recommend(tiny["uids"], 10, diversity=0.7, max_per_artist=2, pool=16, as_ids=False)
    pool_idx = np.full((N_USERS, 16), -1, np.int32)
    pool_score = np.full((N_USERS, 16), -np.inf, np.float32)
    pool_count = np.zeros(N_USERS, np.int32)
    for u in range(N_USERS):
        idx, score = _ranking(tiny["full"], u)
        ci, cs = R.cap_full_ranking(idx[:16], score[:16], g, 2, 16)
        pool_idx[u, :len(ci)], pool_score[u, :len(ci)], pool_count[u] = ci, cs, len(ci)
    k = 10
    want = rank.Diversify(DEV).mmr_raw(torch.from_numpy(pool_idx).to(DEV), torch.from_numpy(pool_score).to(DEV),
                                       torch.from_numpy(pool_count).to(DEV), tr._item_feat_by_index(), k, 0.7)
    want = [t.cpu().numpy() for t in want]
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[2], want[2])
    for u in range(N_USERS):  # every list satisfies the cap
        groups = g[got[0][u, :got[2][u]]]
        assert all((groups == a).sum() <= 2 for a in set(groups[groups >= 0].tolist()))


def test_evaluate_topk_artist_numbers_equal_the_host_reference(tiny):
    tr, g = tiny["tr"], tiny["group_of"]
    ks = (3, 10)
    got = tr.evaluate_topk(ks=ks, artists=True)
    lists = tr.recommend(tiny["uids"], 10, exclude_seen=False, as_ids=False)  # evaluate_topk's lists
    exposure = np.zeros((len(ks), 9), np.int64)
    st, flags = R.stats(lists[0].astype(np.int32), lists[2], g, 9, ks, exposure)
    mean, cov, n = R.stats_mean(st, flags, exposure, np.ones(9, np.uint8))
    assert got["n_artist_lists"] == n == N_USERS and got["n_users"] == N_USERS
    for i, k in enumerate(ks):
        assert got["artists@%d" % k] == mean[i, 0] and got["artist_top@%d" % k] == mean[i, 1]
        assert got["artist_coverage@%d" % k] == cov[i]
    plain = tr.evaluate_topk(ks=ks)
    assert all(got[key] == plain[key] for key in plain)  # the ranking metrics are untouched
    capped = tr.evaluate_topk(ks=ks, artists=True, max_per_artist=1, pool=40)
    assert capped["artist_top@10"] == 1.0 and capped["artists@10"] > got["artists@10"]


def test_wrmf_groups_cap_the_inner_product_lists(tiny):
    """WRMF.recommend / evaluate_topk(groups=, max_per_group=): the same cap over dot-product lists, with
    deepening; without the arguments, today's lists."""
    from dcrecommend.dcbr import WRMF, device_csr
    from dcrecommend.nn import rank
    g, ds = tiny["group_of"], tiny["ds"]
    users, items = _factors()
    ptr, idx = ds.user_item_csr()
    r = torch.as_tensor(np.repeat(np.arange(N_USERS), np.diff(ptr)), device=DEV)
    c = torch.as_tensor(idx.astype(np.int64), device=DEV)
    m = WRMF(factors=D, regularization=0.1, alpha=40.0, iterations=0, device=DEV)
    m.by_user, m.by_item = device_csr(r, c, None, N_USERS), device_csr(c, r, None, N_SONGS)
    m.init_factors(N_USERS, N_SONGS)
    m.user_factors.copy_(torch.from_numpy(users))
    m.item_factors.copy_(torch.from_numpy(items))
    rows = np.arange(N_USERS)
    full = m.recommend(rows, N_SONGS)
    want = [R.cap_full_ranking(*_ranking(full, u), g, 2, 10) for u in rows]
    _assert_lists(m.recommend(rows, 10, groups=g, max_per_group=2, pool=16), [w[0] for w in want], [w[1] for w in want])
    today = rank.TopK(ptr, idx, None, DEV, n_cand=N_SONGS, score="dot").topk(m.user_factors, m.item_factors, rows, 10)
    got = m.recommend(rows, 10)
    assert np.array_equal(got[0], today[0]) and np.array_equal(_bits(got[1]), _bits(today[1]))
    with pytest.raises(ValueError, match="max_per_group"):
        m.recommend(rows, 10, groups=g)
    res = m.evaluate_topk(ptr, idx, ks=(5, 10), groups=g, max_per_group=1, pool=40)
    assert res["group_top@10"] == 1.0 and res["n_group_lists"] == N_USERS and 0 < res["group_coverage@5"] <= 1


def test_defaults_are_todays_path_bit_for_bit(tiny):
    from dcrecommend.nn import rank
    tr, ds = tiny["tr"], tiny["ds"]
    feat = tr._item_feat_by_index()
    mask = np.ones(N_SONGS, np.uint8)
    rows = np.arange(N_USERS)
    today = rank.TopK(*ds.user_item_csr(), mask, DEV).topk(tr.user_factors, feat, rows, 10)
    for got in (tr.recommend(tiny["uids"], 10, as_ids=False), tr.explain(tiny["uids"], 10, reasons=2, as_ids=False)[:3],
                tr._topk("user", None, True).topk(tr.user_factors, feat, rows, 10, group_of=None, max_per_group=None)):
        assert np.array_equal(got[0], today[0]) and np.array_equal(_bits(got[1]), _bits(today[1]))
        assert np.array_equal(got[2], today[2])
    song_rows = np.arange(0, N_SONGS, 7)
    today = rank.TopK(*rank.identity_csr(N_SONGS), mask, DEV).topk(feat, feat, song_rows, 10)
    got = tr.similar_songs([tiny["songs"][r] for r in song_rows], 10)
    assert [[tiny["songs"].index(s) for s, _ in row] for row in got] == today[0].tolist()
    assert np.array_equal(_bits([[x for _, x in row] for row in got]), _bits(today[1]))
    diverse = rank.TopK(*ds.user_item_csr(), mask, DEV).topk(tr.user_factors, feat, rows, 10, diversity=0.6, pool=24)
    got = tr.recommend(tiny["uids"], 10, diversity=0.6, pool=24, as_ids=False)
    assert np.array_equal(got[0], diverse[0]) and np.array_equal(_bits(got[1]), _bits(diverse[1]))
