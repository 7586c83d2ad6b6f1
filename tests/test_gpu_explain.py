"""GPU tests of explained lists (dcue_list_explain, rank.Explain, DCUE.explain / explain_for, WRMF.explain,
train_dcue.py --recommend-reasons) against the numpy reference in explain_reference.py.

Exact cases use test_gpu_mmr's factors (rows in {0, +-1} with 4 or 16 non-zeros: norms 2 or 4, every
cosine a dyadic fraction, exact in fp32 in any summation order), so indices and similarity bits must
equal the fp64 reference's, tie order included. Gaussian cases must carry dcue_topk's own bits (an
item-to-item TopK call over the user's usable history returns the same indices and the same uint32
scores) and are held against fp64 to test_gpu_topk's tol = (rank_dp(d) + 8) 2^-24: the fp32
accumulation bound of a dp-term dot product of unit vectors plus a few ulps for the two normalisations;
near-ties within 2 tol of the m-th best may fall either way, nothing else.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import explain_reference as R
from test_gpu_mmr import _exact_feat
from test_gpu_topk import _datasets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIST_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _tol(d):
    return ((d + 15) // 16 * 16 + 8) * 2.0 ** -24


def _csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


def _explain(lists, counts, queries, ptr, idx, feat, m, mask=None):
    """dcue_list_explain through rank.Explain.explain_raw: numpy (why_idx, why_sim, flags)."""
    from dcrecommend.nn import rank
    out = rank.Explain(DEV).explain_raw(
        torch.from_numpy(np.ascontiguousarray(lists, dtype=np.int32)).to(DEV),
        torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(DEV), queries, ptr, idx,
        feat if torch.is_tensor(feat) else torch.from_numpy(feat).to(DEV), m, hist_mask=mask)
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, want):
    """GPU against the fp64 reference, bit for bit (the reference's values are exact in fp32)."""
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1].astype(np.float32)))


# --------------------------------------------------------------------- (a) exact, bit for bit
@functools.lru_cache(maxsize=None)
def _exact_table(d, n_cand=400):
    rs = np.random.RandomState(77 + d)
    feat = _exact_feat(rs, n_cand, d)
    rows = [np.sort(rs.choice(n_cand, n, replace=False)) for n in HIST_LENGTHS]
    return feat, torch.from_numpy(feat).to(DEV), _csr(rows)


@pytest.mark.parametrize("d", [4, 16, 17, 128, 129, 256])
@pytest.mark.parametrize("k", [1, 2, 16, 17, 63, 64, 65, 128])
def test_exact_cases_match_the_reference_bit_for_bit(k, d):
    """Every history length against every count, m = 1 and m = 8; the many exact ties pin the tie order."""
    feat, feat_dev, (ptr, idx) = _exact_table(d)
    rs = np.random.RandomState(1000 * k + d)
    counts = [k, k - 1, k // 2, 0, k + 5]  # (k + 5: clamped to k)
    queries = np.repeat(np.arange(len(HIST_LENGTHS)), len(counts)).astype(np.int32)
    count = np.tile(np.array(counts, np.int32), len(HIST_LENGTHS))
    lists = np.stack([rs.choice(len(feat), k, replace=False) for _ in queries]).astype(np.int32)
    for m in (1, 8):
        want = R.explain(lists, count, queries, ptr, idx, feat, m)
        got = _explain(lists, count, queries, ptr, idx, feat_dev, m)
        _assert_same(got, want)
        assert np.array_equal(got[2] != 0, np.diff(ptr)[queries] == 0)  # bit 0: the empty history, nothing else


# --------------------------------------------------------------------- (b), (c) Gaussian factors
GAUSS_HIST = (1, 5, 50, 64, 65, 200, 700)


@functools.lru_cache(maxsize=None)
def _gauss(d, n_cand=2000, k=128):
    """Lists of a real TopK.topk_raw at k = 128 for 7 users whose histories (their exclusion rows) have
    1 .. 700 songs, a mask that drops a fifth of the catalogue from every history, and the m = 8 result."""
    from dcrecommend.nn import rank
    rs = np.random.RandomState(5 + d)
    feat = rs.randn(n_cand, d).astype(np.float32)
    users = rs.randn(len(GAUSS_HIST), d).astype(np.float32)
    ptr, idx = _csr([np.sort(rs.choice(n_cand, n, replace=False)) for n in GAUSS_HIST])
    mask = (rs.rand(n_cand) < 0.8).astype(np.uint8)
    mask[idx[ptr[0]]] = 1  # the one-song history stays usable
    feat_dev = torch.from_numpy(feat).to(DEV)
    q = np.arange(len(GAUSS_HIST))
    tk = rank.TopK(ptr, idx, None, DEV, n_cand=n_cand)
    lists, _, count, flags = tk.topk_raw(torch.from_numpy(users).to(DEV), feat_dev, q, k)
    assert int(flags.abs().sum()) == 0 and count.cpu().numpy().tolist() == [k] * len(q)
    got = rank.Explain(DEV).explain_raw(lists, count, q, ptr, idx, feat_dev, 8, hist_mask=mask)
    return dict(feat=feat, feat_dev=feat_dev, ptr=ptr, idx=idx, mask=mask, q=q, lists=lists.cpu().numpy(),
                count=count.cpu().numpy(), got=tuple(t.cpu().numpy() for t in got), d=d, k=k)


@pytest.mark.parametrize("d", [16, 100, 128, 256])
def test_reasons_carry_dcue_topk_bits(d):
    """For the first, middle and last pick of each list, one item-to-item TopK call per list (cand_mask =
    the user's usable history, no exclusion, k = 8) returns the same indices and the same score bits."""
    from dcrecommend.nn import rank
    c = _gauss(d)
    why_idx, why_sim, flags = c["got"]
    assert not flags.any()
    for u in c["q"]:
        H, _ = R.history(u, c["ptr"], c["idx"], len(c["feat"]), c["mask"])
        usable = np.zeros(len(c["feat"]), np.uint8)
        usable[H] = 1
        pos = [0, c["k"] // 2, c["k"] - 1]
        picks = c["lists"][u, pos]
        tk = rank.TopK(None, None, usable, DEV)
        idx, score, count, tflags = [t.cpu().numpy() for t in tk.topk_raw(c["feat_dev"], c["feat_dev"], picks, 8)]
        assert not tflags.any() and count.tolist() == [min(8, len(H))] * 3
        assert np.array_equal(idx, why_idx[u, pos]), (d, u)
        assert np.array_equal(_bits(score), _bits(why_sim[u, pos])), (d, u)


@pytest.mark.parametrize("d", [16, 100, 128, 256])
def test_gaussian_vs_fp64(d):
    c = _gauss(d)
    why_idx, why_sim, flags = c["got"]
    assert not flags.any()
    for u in c["q"]:
        R.check_tolerant(why_idx[u], why_sim[u], c["lists"][u], c["count"][u], int(u), c["ptr"], c["idx"], c["feat"], 8,
                         _tol(d), c["mask"])


# --------------------------------------------------------------------- (d) invariance
@pytest.mark.parametrize("d", [100, 256])
def test_invariant_to_batching_order_and_csr_offset(d):
    c = _gauss(d)
    n = len(c["q"])
    args = (c["ptr"], c["idx"], c["feat_dev"], 8, c["mask"])
    for u in range(n):  # every list alone
        one = _explain(c["lists"][u:u + 1], c["count"][u:u + 1], c["q"][u:u + 1], *args)
        assert np.array_equal(one[0][0], c["got"][0][u]) and np.array_equal(_bits(one[1][0]), _bits(c["got"][1][u]))
        assert one[2][0] == c["got"][2][u]
    rev = _explain(c["lists"][::-1], c["count"][::-1], c["q"][::-1], *args)  # reversed order
    assert np.array_equal(rev[0][::-1], c["got"][0]) and np.array_equal(_bits(rev[1][::-1]), _bits(c["got"][1]))
    # the same histories at other offsets of a larger CSR: rows in reversed order behind a 37-entry row
    rows = [c["idx"][c["ptr"][u]:c["ptr"][u + 1]] for u in range(n)]
    ptr2, idx2 = _csr([np.arange(37)] + rows[::-1])
    moved = _explain(c["lists"], c["count"], n - c["q"], ptr2, idx2, c["feat_dev"], 8, c["mask"])
    assert np.array_equal(moved[0], c["got"][0]) and np.array_equal(_bits(moved[1]), _bits(c["got"][1]))
    assert np.array_equal(moved[2], c["got"][2])


# --------------------------------------------------------------------- (e) mask and flags
def test_masked_entries_are_never_returned():
    c = _gauss(100)
    why_idx = c["got"][0]
    assert np.all(c["mask"][why_idx[why_idx >= 0]] == 1)
    for u in c["q"]:
        row = c["idx"][c["ptr"][u]:c["ptr"][u + 1]]
        assert np.isin(why_idx[u][why_idx[u] >= 0], row).all()
    # an all-masked history: bit 0, all padding
    mask = c["mask"].copy()
    mask[c["idx"][c["ptr"][1]:c["ptr"][2]]] = 0
    got = _explain(c["lists"], c["count"], c["q"], c["ptr"], c["idx"], c["feat_dev"], 8, mask)
    assert got[2][1] == R.FLAG_NO_HISTORY and np.all(got[0][1] == -1) and np.all(np.isneginf(got[1][1]))
    _assert_masked_equals_reference_order(got, c, mask)


def _assert_masked_equals_reference_order(got, c, mask):
    for u in c["q"]:
        if got[2][u] == 0:
            R.check_tolerant(got[0][u], got[1][u], c["lists"][u], c["count"][u], int(u), c["ptr"], c["idx"], c["feat"],
                             8, _tol(c["d"]), mask)


@pytest.mark.parametrize("what", ["list", "history", "query"])
def test_bad_index_flags_only_its_own_list(what):
    c = _gauss(100)
    n_cand, victim = len(c["feat"]), 3
    lists, ptr, idx, q = c["lists"].copy(), c["ptr"], c["idx"].copy(), c["q"].copy()
    if what == "list":
        lists[victim, 77] = n_cand  # (the second pass of a 128-pick list)
    elif what == "history":
        idx[ptr[victim + 1] - 1] = n_cand + 5  # (the last entry: the row stays sorted)
    else:
        q[victim] = len(ptr) - 1
    got = _explain(lists, c["count"], q, ptr, idx, c["feat_dev"], 8, c["mask"])
    assert got[2][victim] == R.FLAG_BAD_INDEX and np.all(got[0][victim] == -1) and np.all(np.isneginf(got[1][victim]))
    others = np.arange(len(q)) != victim
    assert not got[2][others].any()
    assert np.array_equal(got[0][others], c["got"][0][others])
    assert np.array_equal(_bits(got[1][others]), _bits(c["got"][1][others]))
    if what == "query":
        q[victim] = -1
        assert _explain(lists, c["count"], q, ptr, idx, c["feat_dev"], 8, c["mask"])[2][victim] == R.FLAG_BAD_INDEX
    if what == "list":  # past the count the entry is never read
        count = c["count"].copy()
        count[victim] = 77
        got = _explain(lists, count, q, ptr, idx, c["feat_dev"], 8, c["mask"])
        assert got[2][victim] == 0 and np.array_equal(got[0][victim, :77], c["got"][0][victim, :77])
        assert np.all(got[0][victim, 77:] == -1) and np.all(np.isneginf(got[1][victim, 77:]))


def test_nan_rows():
    c = _gauss(100)
    u = 4  # 65 songs
    H, _ = R.history(u, c["ptr"], c["idx"], len(c["feat"]), c["mask"])
    song = next(int(h) for h in H[len(H) // 2:] if not (c["lists"] == h).any())  # in a history, in no list
    feat = c["feat"].copy()
    feat[song, 3] = np.nan
    got = _explain(c["lists"], c["count"], c["q"], c["ptr"], c["idx"], torch.from_numpy(feat).to(DEV), 8, c["mask"])
    # a NaN row in a history is never returned and sets bit 2 for the lists whose history has it ...
    has = np.array([song in R.history(v, c["ptr"], c["idx"], len(feat), c["mask"])[0] for v in c["q"]])
    assert has[u] and np.array_equal(got[2] == R.FLAG_NONFINITE, has) and not got[2][~has].any()
    assert not (got[0] == song).any() and not np.isnan(got[1]).any()
    # ... and the other reasons equal the run with that song masked
    mask = c["mask"].copy()
    mask[song] = 0
    want = _explain(c["lists"], c["count"], c["q"], c["ptr"], c["idx"], c["feat_dev"], 8, mask)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])) and not want[2].any()
    # a NaN row as a pick leaves that row all padding and the list's other rows intact
    pick = int(c["lists"][2, 70])
    feat = c["feat"].copy()
    feat[pick, 0] = np.nan
    in_hist = np.array([pick in R.history(v, c["ptr"], c["idx"], len(feat), c["mask"])[0] for v in c["q"]])
    got = _explain(c["lists"], c["count"], c["q"], c["ptr"], c["idx"], torch.from_numpy(feat).to(DEV), 8, c["mask"])
    assert got[2][2] == R.FLAG_NONFINITE and np.all(got[0][2, 70] == -1) and np.all(np.isneginf(got[1][2, 70]))
    rest = np.arange(c["k"]) != 70
    assert np.array_equal(got[0][2, rest], c["got"][0][2, rest])
    assert np.array_equal(_bits(got[1][2, rest]), _bits(c["got"][1][2, rest]))
    for v in c["q"]:
        named = (c["lists"][v] == pick).any() or in_hist[v]
        assert (got[2][v] == R.FLAG_NONFINITE) == bool(named)


# --------------------------------------------------------------------- (f) MMR input
def test_mmr_output_is_accepted():
    from dcrecommend.nn import rank
    c = _gauss(128)
    rs = np.random.RandomState(9)
    users = torch.from_numpy(rs.randn(len(c["q"]), 128).astype(np.float32)).to(DEV)
    tk = rank.TopK(c["ptr"], c["idx"], None, DEV, n_cand=len(c["feat"]))
    lists, _, count, _ = tk.topk_raw(users, c["feat_dev"], c["q"], 20, diversity=0.5, pool=80)
    why_idx, why_sim, flags = [t.cpu().numpy() for t in rank.Explain(DEV).explain_raw(
        lists, count, c["q"], c["ptr"], c["idx"], c["feat_dev"], 3, hist_mask=c["mask"])]
    assert not flags.any() and why_idx.shape == (len(c["q"]), 20, 3)
    lists, count = lists.cpu().numpy(), count.cpu().numpy()
    for u in c["q"]:
        R.check_tolerant(why_idx[u], why_sim[u], lists[u], count[u], int(u), c["ptr"], c["idx"], c["feat"], 3, _tol(128),
                         c["mask"])


# --------------------------------------------------------------------- (g) surface
@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    """test_gpu_topk's tiny synthetic fit."""
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


def _raw_reasons(tr, idx, count, rows, ptr, hidx, m):
    """The raw call on lists given as arrays: what the surface must agree with."""
    return _explain(idx, count, rows, ptr, hidx, tr._item_feat_by_index(), m, (tr._item_meta >= 0).astype(np.uint8))


@pytest.mark.parametrize("kw", [dict(), dict(dataset="val"), dict(exclude_seen=False), dict(diversity=0.6, pool=16)])
def test_dcue_explain(trained, kw):
    g, tr, train, val = trained
    kw = dict(kw, dataset=val) if "dataset" in kw else kw
    users = list(g["val_users"][:6])
    idx, score, count, why_idx, why_sim = tr.explain(users, k=7, reasons=3, as_ids=False, **kw)
    ridx, rscore, rcount = tr.recommend(users, k=7, as_ids=False, **kw)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(score), _bits(rscore)) and np.array_equal(count, rcount)
    ptr, seen = train.user_item_csr()
    rows = np.array([train.user_index[u] for u in users])
    raw = _raw_reasons(tr, idx, count, rows, ptr, seen, 3)
    assert np.array_equal(why_idx, raw[0]) and np.array_equal(_bits(why_sim), _bits(raw[1]))
    for r, ui in enumerate(rows):  # every reason is a song of the user's history that has audio
        got = why_idx[r][why_idx[r] >= 0]
        assert len(got) and np.isin(got, seen[ptr[ui]:ptr[ui + 1]]).all() and np.all(tr._item_meta[got] >= 0)
    src = val if "dataset" in kw else train
    names = src.itemindex2songid
    lists = tr.explain(users, k=7, reasons=3, **kw)
    for r, lst in enumerate(lists):
        assert [p[0] for p in lst] == [names[int(i)] for i in idx[r, :count[r]]]
        assert [p[1] for p in lst] == [float(s) for s in score[r, :count[r]]]
        for j, (_, _, why) in enumerate(lst):
            keep = why_idx[r, j] >= 0
            assert why == [(names[int(h)], float(s)) for h, s in zip(why_idx[r, j][keep], why_sim[r, j][keep])]
    with pytest.raises(ValueError, match=r"1\.\.8"):
        tr.explain(users, k=7, reasons=9)
    with pytest.raises(KeyError):
        tr.explain(["no such user"], k=7)


def test_dcue_explain_for(trained):
    g, tr, train, val = trained
    ptr, seen = train.user_item_csr()
    names = train.itemindex2songid
    rows = [train.user_index[u] for u in g["val_users"][:3]]
    histories = [[names[int(i)] for i in seen[ptr[ui]:ptr[ui + 1]]] for ui in rows]
    idx, score, count, why_idx, why_sim = tr.explain_for(histories, k=6, reasons=2, as_ids=False, steps=5)
    ridx, rscore, rcount = tr.recommend_for(histories, k=6, as_ids=False, steps=5)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(score), _bits(rscore)) and np.array_equal(count, rcount)
    usable, _ = tr._history_items(histories, None)
    hp, hi = _csr([np.array(u) for u in usable])
    raw = _raw_reasons(tr, idx, count, np.arange(3), hp, hi, 2)
    assert np.array_equal(why_idx, raw[0]) and np.array_equal(_bits(why_sim), _bits(raw[1]))
    lists = tr.explain_for(histories, k=6, reasons=2, steps=5)
    for r, lst in enumerate(lists):
        assert [p[0] for p in lst] == [names[int(i)] for i in idx[r, :count[r]]]
        assert all(h in histories[r] for _, _, why in lst for h, _ in why)


def test_wrmf_explain():
    from dcrecommend.dcbr.wrmf import WRMF
    rs = np.random.RandomState(3)
    n_users, n_items = 40, 90
    pairs = sorted({(int(rs.randint(n_users)), int(rs.randint(n_items))) for _ in range(600)})
    rows, cols = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    m = WRMF(factors=16, regularization=0.1, alpha=40.0, iterations=2, seed=2, device=DEV)
    m.fit(rows, cols, rs.randint(1, 5, len(pairs)).astype(np.float32), n_users=n_users, n_items=n_items)
    users = [0, 5, 17, 39]
    idx, score, count, why_idx, why_sim = m.explain(users, k=9, reasons=4)
    ridx, rscore, rcount = m.recommend(users, k=9)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(score), _bits(rscore)) and np.array_equal(count, rcount)
    ptr, hidx = _csr([np.sort(cols[rows == u]) for u in range(n_users)])
    raw = _explain(idx, count, users, ptr, hidx, m.item_factors, 4)
    assert np.array_equal(why_idx, raw[0]) and np.array_equal(_bits(why_sim), _bits(raw[1])) and not raw[2].any()
    feat = m.item_factors.cpu().numpy()
    for r, u in enumerate(users):
        R.check_tolerant(why_idx[r], why_sim[r], idx[r], count[r], u, ptr, hidx, feat, 4, _tol(16))


def test_train_dcue_driver_writes_reasons(tmp_path):
    import train_dcue
    out, why = tmp_path / "rec.csv", tmp_path / "why.csv"
    argv = ["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80", "--synthetic-pairs", "300",
            "--feature-dim", "32", "--conv-hidden", "32", "--batch-size", "8", "--neg-batch-size", "3",
            "--num-epochs", "1", "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path / "ck"),
            "--recommend-k", "5", "--recommend-out", str(out), "--recommend-reasons", "2", "--reasons-out", str(why)]
    dcue = train_dcue.main(argv)
    rec, rs = pd.read_csv(out), pd.read_csv(why)
    assert list(rec.columns) == ["user_id", "rank", "song_id", "score"]
    assert list(rs.columns) == ["user_id", "rank", "song_id", "reason_rank", "reason_song_id", "similarity"]
    users = list(dcue.train_data.uniq_users)
    lists = dcue.explain(users, k=5, reasons=2)  # the raw call behind the driver, on the same factors
    want = [(u, r + 1, song, j + 1, h, s) for u, lst in zip(users, lists) for r, (song, _, because) in enumerate(lst)
            for j, (h, s) in enumerate(because)]
    assert len(want) == len(rs) > 0
    assert [tuple(x) for x in rs[["user_id", "rank", "song_id", "reason_rank", "reason_song_id"]].values.tolist()] \
        == [w[:5] for w in want]
    assert np.array_equal(_bits(rs["similarity"].to_numpy()), _bits([w[5] for w in want]))
    assert rec[["user_id", "rank", "song_id"]].values.tolist() \
        == [[u, r + 1, song] for u, lst in zip(users, lists) for r, (song, _, _) in enumerate(lst)]
    coo = dcue.train_data.item_user.tocoo()
    played = set((dcue.train_data.userindex2userid[c], dcue.train_data.itemindex2songid[r])
                 for r, c in zip(coo.row, coo.col))
    assert all((u, h) in played for u, h in zip(rs["user_id"], rs["reason_song_id"]))
