"""Host-side tests of artist-aware serving: the library's symbols and host refusals (dcue_list_group_cap,
dcue_list_group_stats, dcue_list_group_stats_mean validate every argument before their first device call,
so they answer without a GPU), datasets.artists against brute-force set constructions, the Python
argument errors, and DCUEDataset's artist split."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from dcrecommend import _native as nat

INVALID, UNSUPPORTED = 1, 2
P = ctypes.c_void_p(64)  # a non-null pointer that a refused call never reads


def _err():
    return nat.lib().dcue_last_error().decode()


def _cap(**kw):
    a = dict(idx=P, score=P, count=P, n=4, pool=16, group_of=P, n_cand=100, n_groups=5, cap=2, k_out=8,
             cidx=None, cscore=None, ccount=None, oidx=P, oscore=P, ocount=P, dropped=None, flags=P)
    a.update(kw)
    return nat.lib().dcue_list_group_cap(a["idx"], a["score"], a["count"], a["n"], a["pool"], a["group_of"],
                                         a["n_cand"], a["n_groups"], a["cap"], a["k_out"], a["cidx"], a["cscore"],
                                         a["ccount"], a["oidx"], a["oscore"], a["ocount"], a["dropped"], a["flags"],
                                         None)


def _stats(cutoffs=(1, 5), **kw):
    cut = (ctypes.c_int32 * max(len(cutoffs), 1))(*cutoffs)
    a = dict(idx=P, count=P, n=4, k=16, group_of=P, n_cand=100, n_groups=5, cut=ctypes.cast(cut, ctypes.c_void_p),
             m=len(cutoffs), out=P, flags=P, exposure=None)
    a.update(kw)
    return nat.lib().dcue_list_group_stats(a["idx"], a["count"], a["n"], a["k"], a["group_of"], a["n_cand"],
                                           a["n_groups"], a["cut"], a["m"], a["out"], a["flags"], a["exposure"], None)


def test_symbols_and_constants():
    lib = nat.lib()
    for name in ("dcue_list_group_cap", "dcue_list_group_stats", "dcue_list_group_stats_mean"):
        assert hasattr(lib, name) and name in nat._SIGS
    assert (nat.GROUP_FLAG_SHORT, nat.GROUP_FLAG_BAD_GROUP, nat.GROUP_N_STATS) == (8, 16, 2)
    assert nat.LIST_FLAG_BAD_INDEX == 2 and nat.TOPK_MAX_K == 128
    header = open(nat.LIB_PATH.rsplit("/amplifai", 1)[0] + "/include/dcue.h").read()
    for text in ("#define DCUE_GROUP_FLAG_SHORT 8", "#define DCUE_GROUP_FLAG_BAD_GROUP 16", "#define DCUE_ABI_VERSION 17"):
        assert text in header


@pytest.mark.parametrize("kw, code, word", [
    (dict(idx=None), INVALID, "null"), (dict(score=None), INVALID, "null"), (dict(count=None), INVALID, "null"),
    (dict(group_of=None), INVALID, "null"), (dict(oidx=None), INVALID, "null"), (dict(oscore=None), INVALID, "null"),
    (dict(ocount=None), INVALID, "null"), (dict(flags=None), INVALID, "null"),
    (dict(cap=0), INVALID, "cap"), (dict(cap=-3), INVALID, "cap"),
    (dict(k_out=0), INVALID, "k_out"), (dict(k_out=129), INVALID, "k_out"),
    (dict(pool=0), INVALID, "pool"), (dict(pool=129), INVALID, "pool"),
    (dict(n=-1), INVALID, "n_lists"), (dict(n_groups=-1), INVALID, "n_groups"), (dict(n_cand=0), INVALID, "n_cand"),
    (dict(n_cand=2 ** 31 - 10), UNSUPPORTED, "bound"),
    (dict(cidx=P), INVALID, "carry"), (dict(cidx=P, cscore=P), INVALID, "carry"), (dict(ccount=P), INVALID, "carry"),
    (dict(cscore=P, ccount=P), INVALID, "carry"),
])
def test_cap_host_refusals(kw, code, word):
    assert _cap(**kw) == code
    assert "dcue_list_group_cap" in _err() and word in _err()


def test_empty_launches_are_ok():
    assert _cap(n=0) == 0 and _cap(n=0, cidx=P, cscore=P, ccount=P, dropped=P) == 0
    assert _stats(n=0) == 0


@pytest.mark.parametrize("kw, cutoffs, code, word", [
    (dict(idx=None), (1,), INVALID, "null"), (dict(count=None), (1,), INVALID, "null"),
    (dict(group_of=None), (1,), INVALID, "null"), (dict(out=None), (1,), INVALID, "null"),
    (dict(flags=None), (1,), INVALID, "null"), (dict(cut=None), (1,), INVALID, "null"),
    (dict(k=0), (1,), INVALID, "1..128"), (dict(k=129), (1,), INVALID, "1..128"),
    (dict(), (), INVALID, "n_cutoffs"), (dict(), tuple(range(1, 10)), INVALID, "n_cutoffs"),
    (dict(), (0, 3), INVALID, "cutoffs"), (dict(), (3, 3), INVALID, "cutoffs"), (dict(), (5, 2), INVALID, "cutoffs"),
    (dict(), (4, 17), INVALID, "cutoffs"), (dict(n_groups=-2), (1,), INVALID, "n_groups"),
    (dict(n_cand=2 ** 31 - 10), (1,), UNSUPPORTED, "bound"),
])
def test_stats_host_refusals(kw, cutoffs, code, word):
    assert _stats(cutoffs, **kw) == code
    assert "dcue_list_group_stats" in _err() and word in _err()


def test_stats_mean_host_refusals():
    mean = nat.lib().dcue_list_group_stats_mean
    assert mean(None, P, 4, 2, None, None, 0, P, None, P, None) == INVALID and "null" in _err()
    assert mean(P, P, 4, 2, None, None, 0, None, None, P, None) == INVALID and "null" in _err()
    assert mean(P, P, 4, 2, P, None, 5, P, None, P, None) == INVALID and "go together" in _err()
    assert mean(P, P, 4, 2, None, None, 5, P, P, P, None) == INVALID and "go together" in _err()
    assert mean(P, P, 4, 0, None, None, 0, P, None, P, None) == INVALID and "n_cutoffs" in _err()
    assert mean(P, P, 4, 9, None, None, 0, P, None, P, None) == INVALID and "n_cutoffs" in _err()
    assert mean(P, P, -1, 2, None, None, 0, P, None, P, None) == INVALID and "negative" in _err()


# ----------------------------------------------------------------------------- datasets.artists
def test_artist_groups_order_and_missing():
    from dcrecommend.datasets.artists import artist_groups
    item_index = {"s%02d" % i: i for i in range(7)}
    amap = {"s00": "Zed", "s01": "abba", "s02": "Mia", "s04": "Zed", "s05": None, "s06": "Mia", "elsewhere": "Aaa"}
    group_of, names = artist_groups(item_index, amap)
    assert names == ["Mia", "Zed", "abba"]  # sorted; only the artists present ("Aaa" has no song here)
    assert group_of.dtype == np.int32 and group_of.tolist() == [1, 2, 0, -1, 1, -1, 0]
    with pytest.raises(ValueError):
        artist_groups({"a": 0, "b": 0}, amap)


def _rows(ptr, idx):
    return [idx[ptr[r]:ptr[r + 1]].tolist() for r in range(len(ptr) - 1)]


def test_exclusion_csrs_match_set_construction():
    from dcrecommend.datasets.artists import artist_exclusion_csr
    from dcrecommend.nn.rank import histories_csr, identity_csr
    rs = np.random.RandomState(3)
    n, n_users = 60, 25
    group_of = rs.randint(-1, 7, n).astype(np.int32)
    played = [np.unique(rs.choice(n, rs.randint(0, 9))) for _ in range(n_users)]
    hist = histories_csr(played)
    same = lambda i: {j for j in range(n) if group_of[i] >= 0 and group_of[j] == group_of[i]}

    ptr, idx = artist_exclusion_csr(group_of)  # per song: the other songs of its artist
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert _rows(ptr, idx) == [sorted(same(i) - {i}) for i in range(n)]
    ptr, idx = artist_exclusion_csr(group_of, seen=identity_csr(n))  # ... and the song itself
    assert _rows(ptr, idx) == [sorted(same(i) | {i}) for i in range(n)]

    by_artist = [set().union(*[same(i) for i in row]) if len(row) else set() for row in played]
    ptr, idx = artist_exclusion_csr(group_of, played=hist)  # per user: every song of the played artists
    assert _rows(ptr, idx) == [sorted(s) for s in by_artist]
    ptr, idx = artist_exclusion_csr(group_of, played=hist, seen=hist)  # ... united with the seen songs
    want = [sorted(s | set(row.tolist())) for s, row in zip(by_artist, played)]
    assert _rows(ptr, idx) == want
    assert all(r == sorted(set(r)) for r in _rows(ptr, idx))
    assert any(group_of[i] < 0 for row in played for i in row)  # ungrouped played songs: in by `seen` only


# ----------------------------------------------------------------------------- Python argument errors
def test_python_argument_errors():
    import torch
    from dcrecommend.nn import rank
    from dcrecommend.nn.dcue import DCUE
    tk = rank.TopK(None, None, None, "cpu", n_cand=10)
    f = torch.zeros(4, 8)
    g = np.zeros(10, np.int32)
    with pytest.raises(ValueError, match="cap_rounds"):
        tk.topk_raw(f, f, [0], 3, group_of=g, max_per_group=2, cap_rounds=0)
    with pytest.raises(ValueError, match="max_per_group"):
        tk.topk_raw(f, f, [0], 3, group_of=g, max_per_group=0)
    with pytest.raises(ValueError, match="group_of"):
        tk.topk_raw(f, f, [0], 3, max_per_group=2)
    with pytest.raises(ValueError, match="group_of"):
        tk.topk_raw(f, f, [0], 3, group_of=g)
    with pytest.raises(ValueError, match="10 candidates"):
        tk.topk_raw(f, f, [0], 3, group_of=g[:5], max_per_group=2)
    with pytest.raises(ValueError, match="pool"):
        tk.topk_raw(f, f, [0], 3, pool=16)  # pool without a cap or diversity
    with pytest.raises(ValueError, match="pool"):
        tk.topk_raw(f, f, [0], 8, pool=4, group_of=g, max_per_group=2)  # pool below k

    tr = DCUE(feature_dim=8, device="cpu")
    tr.user_factors, tr.item_factors, tr._item_meta = f, f, np.arange(4)

    class Src:
        user_index, item_index = {"u": 0}, {"s%d" % i: i for i in range(4)}
    tr.train_data = Src()
    with pytest.raises(RuntimeError, match="set_artists"):
        tr.recommend(["u"], 2, max_per_artist=2)
    with pytest.raises(RuntimeError, match="set_artists"):
        tr.recommend_artists(["u"], 2)
    with pytest.raises(RuntimeError, match="set_artists"):
        tr.similar_songs(["s0"], 2, other_artists=True)
    tr.set_artists({"s0": "a", "s1": "a"})
    assert tr._artist_groups(None)[0].tolist() == [0, 0, -1, -1] and tr._artist_groups(None)[1] == ["a"]


def test_cli_artist_flags():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train_dcue
    base = ["--synthetic"]
    rec = base + ["--recommend-k", "5", "--recommend-out", "r.csv"]
    a = train_dcue.parse(rec)
    assert a.artists is None and a.recommend_max_per_artist is None and not a.recommend_new_artists
    assert a.recommend_artists_out is None and not a.eval_artists
    a = train_dcue.parse(rec + ["--artists", "a.csv", "--recommend-max-per-artist", "2", "--recommend-pool", "20",
                                "--recommend-new-artists", "--recommend-artists-out", "o.csv", "--eval-k", "5",
                                "--eval-out", "m.json", "--eval-artists"])
    assert (a.artists, a.recommend_max_per_artist, a.recommend_pool, a.recommend_new_artists,
            a.recommend_artists_out, a.eval_artists) == ("a.csv", 2, 20, True, "o.csv", True)
    for bad in (rec + ["--recommend-max-per-artist", "2"], rec + ["--recommend-new-artists"],
                rec + ["--recommend-artists-out", "o.csv"], base + ["--artists", "a.csv", "--eval-artists"],
                base + ["--artists", "a.csv", "--recommend-max-per-artist", "2"],
                rec + ["--artists", "a.csv", "--recommend-max-per-artist", "0"], rec + ["--recommend-pool", "20"],
                rec + ["--artists", "a.csv", "--recommend-artists-out", "o.csv", "--recommend-for", "n.csv"]):
        with pytest.raises(SystemExit):
            train_dcue.parse(bad)


# ----------------------------------------------------------------------------- the artist split
def _frame(seed=0, n_songs=90, n_artists=14, n_users=12):
    rs = np.random.RandomState(seed)
    songs = ["S%03d" % i for i in range(n_songs)]
    amap = {s: "A%02d" % rs.randint(n_artists) for s in songs}
    rows = [(u, s) for u in range(n_users) for s in rs.choice(songs, 25, replace=False)]
    rows += [(0, s) for s in songs]  # every song appears
    trip = pd.DataFrame({"user_id": ["U%02d" % u for u, _ in rows], "song_id": [s for _, s in rows], "score": 1.0})
    trip = trip.drop_duplicates(["user_id", "song_id"]).reset_index(drop=True)
    meta = pd.DataFrame({"idx": np.arange(n_songs), "song_id": songs, "data_mel": ["x"] * n_songs})
    return trip, meta, amap


def _split_songs(split, amap, seed=0):
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    trip, meta, _ = _frame(seed)
    return set(DCUEDataset(trip, meta, split=split, song_artist_map=amap).triplets["song_id"].astype(str))


def test_artist_split_partitions_songs_and_keeps_artists_apart():
    trip, _, amap = _frame()
    parts = {s: _split_songs(s, amap) for s in ("train", "val", "test")}
    assert all(len(p) for p in parts.values())
    assert parts["train"] | parts["val"] | parts["test"] == set(trip["song_id"])
    assert sum(len(p) for p in parts.values()) == trip["song_id"].nunique()  # disjoint
    artists = {s: {amap[x] for x in p} for s, p in parts.items()}
    assert not (artists["train"] & artists["val"] or artists["train"] & artists["test"] or artists["val"] & artists["test"])
    assert len(parts["train"]) > len(parts["test"]) > len(parts["val"])  # 70 / 20 / 10 of the artists
    again = {s: _split_songs(s, amap) for s in ("train", "val", "test")}
    assert again == parts  # identical across two constructions
    assert _split_songs("all", amap) == set(trip["song_id"])


def test_mapless_split_and_numpy_stream_are_unchanged():
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    trip, meta, _ = _frame()
    songs = trip["song_id"].astype("category").astype(str).unique()
    got = {}
    for split in ("train", "val", "test"):
        np.random.seed(1234)
        ds = DCUEDataset(trip.copy(), meta, split=split)
        after = np.random.rand(3)
        # where the song split leaves the stream: seed 10, then one draw per train song
        np.random.seed(10)
        in_train = np.random.rand(len(songs)) < 0.80
        np.random.seed(10)
        in_val = np.random.rand(int(in_train.sum())) < 0.1 / 0.8
        assert np.array_equal(after, np.random.rand(3))
        got[split] = set(ds.triplets["song_id"].astype(str))
    train, val = songs[in_train], songs[in_train][in_val]
    assert got == {"train": set(train) - set(val), "val": set(val), "test": set(songs) - set(train)}
