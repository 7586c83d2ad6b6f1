"""Host side of popularity-aware serving (include/dcue.h dcue_topk_prior, dcue_list_item_stats,
dcue_exposure_gini; datasets/popularity.py), no GPU needed: the restatements of popularity_reference.py
against brute force, every refusal of the three new calls (they validate on the host before their first
device call), the 2^53 rule, and DCUE.set_popularity's arrays on a hand example."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import popularity_reference as P

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


# ------------------------------------------------------------------------------- the restatements
def test_topk_prior_against_brute_force():
    s0 = np.array([[0.5, 0.5, 0.25, -0.0, 0.75, 0.5],
                   [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]], np.float32)
    prior = np.array([0.0, 0.0, 0.5, 0.0, -0.5, 0.25], np.float32)
    ptr, idx = np.array([0, 1, 1], np.int64), np.array([5], np.int32)  # row 0 excludes candidate 5
    mask = np.array([1, 1, 1, 1, 1, 1], np.uint8)
    got = P.topk_prior(s0, prior, [0, 1], 4, ptr, idx, mask)
    # row 0 sums: .5 .5 .75 0 .25 (.75 excluded) -> 2, then the tie 0 < 1, then 4
    assert got[0][0].tolist() == [2, 0, 1, 4] and got[1][0].tolist() == [0.75, 0.5, 0.5, 0.25]
    # row 1 sums: .1 .2 .8 .4 0 .85
    assert got[0][1].tolist() == [5, 2, 3, 1]
    assert got[2].tolist() == [4, 4] and not got[3].any()
    for i in range(2):  # brute force: sort (-(s0 + p), index) over the eligible
        items = sorted((-float(np.float32(s0[i, c]) + np.float32(prior[c])), c) for c in range(6)
                       if not (i == 0 and c == 5))
        assert got[0][i].tolist() == [c for _, c in items[:4]]
    # -0 is folded on both sides of the addition: one key per value
    z = P.prior_scores(np.array([[-0.0, 0.0]], np.float32), np.array([-0.0, -0.0], np.float32))
    assert not np.signbit(z).any()
    # a NaN prior on an eligible candidate flags and is never selected; a masked one is not looked at
    bad = prior.copy()
    bad[1] = np.nan
    got = P.topk_prior(s0, bad, [0, 1], 6, ptr, idx, mask)
    assert got[3].all() and not (got[0] == 1).any() and got[2].tolist() == [4, 5]
    mask2 = mask.copy()
    mask2[1] = 0
    assert not P.topk_prior(s0, bad, [0, 1], 6, ptr, idx, mask2)[3].any()
    # overflow of the sum flags too; +inf orders as an ordinary value
    big = np.array([[3e38, 1.0]], np.float32)
    got = P.topk_prior(big, np.array([3e38, 0.0], np.float32), [0], 2)
    assert got[3].all() and got[0][0].tolist() == [0, 1] and np.isposinf(got[1][0, 0])


def test_item_stats_restatement():
    value = np.array([1.0, 2.0, 4.0, 8.0, 0.5], np.float64)
    tail = np.array([0, 1, 1, 0, 7], np.uint8)
    idx = np.array([[3, 1, 4, 0], [2, -1, -1, -1], [0, 0, 0, 0], [1, 9, 0, 0], [1, 9, 0, 0]], np.int32)
    count = np.array([4, 1, 0, 4, 1], np.int32)
    stats, flags = P.item_stats(idx, count, [1, 3, 4], value, tail, 5)
    assert flags.tolist() == [0, 0, 1, 2, 0]  # empty; an out-of-range entry inside the count; outside it
    assert stats[0].tolist() == [[8.0, 0.0], [(8.0 + 2.0 + 0.5) / 3, 2 / 3], [11.5 / 4, 0.5]]
    assert stats[1].tolist() == [[4.0, 1.0]] * 3  # n_K = min(K, 1)
    assert not stats[2].any() and not stats[3].any()
    assert stats[4].tolist() == [[2.0, 1.0]] * 3
    none, _ = P.item_stats(idx, count, [2], None, None, 5)
    assert not none.any()
    mean, ne = P.col_mean(stats.reshape(5, -1), flags)
    assert ne == 3
    np.testing.assert_allclose(mean, stats[[0, 1, 4]].reshape(3, -1).mean(0), rtol=1e-15)


def test_gini_restatement_against_brute_force():
    rs = np.random.RandomState(3)
    for n in (1, 2, 7, 40):
        x = rs.randint(0, 6, n)
        g, total = P.gini(x[None, :])
        num, den = P.gini_brute(x)
        assert total[0] == x.sum()
        assert g[0] == (float(Fraction(num, den)) if den else 0.0) or abs(g[0] - num / den) < 1e-15
    # all exposure on one of n candidates: (n - 1) / n; equal exposure: 0; none: 0
    assert P.gini(np.array([[0, 0, 9, 0]]))[0][0] == 0.75
    assert P.gini(np.array([[3, 3, 3]]))[0][0] == 0.0
    assert P.gini(np.zeros((1, 5), np.int64))[0][0] == 0.0
    # cutoffs cumulate; the mask removes candidates (their exposure with them)
    e = np.array([[4, 0, 0, 0], [0, 4, 0, 0]])
    g, total = P.gini(e)
    assert g.tolist() == [0.75, 0.5] and total.tolist() == [4, 8]
    g, total = P.gini(e, np.array([0, 1, 1, 1], np.uint8))
    assert g.tolist() == [0.0, 2 / 3] and total.tolist() == [0, 4]


def test_host_formulas_against_the_restatement():
    from dcrecommend.datasets import popularity as H
    rs = np.random.RandomState(5)
    for counts in ([7, 0, 1, 3, 1, 0, 0, 15], rs.randint(0, 50, 200).tolist(), [0, 0, 0], [5]):
        np.testing.assert_allclose(H.log_popularity(counts), P.log_popularity(counts), rtol=4e-16, atol=0)
        np.testing.assert_allclose(H.self_information(counts), P.self_information(counts), rtol=4e-16, atol=0)
        for mass in (0.8, 0.5, 0.0, 1.0):
            assert np.array_equal(H.tail_bytes(counts, mass), P.tail_bytes(counts, mass)), (counts, mass)
    z = H.log_popularity([7, 0, 1, 3])
    assert z.tolist() == [1.0, 0.0, 1.0 / 3.0, 2.0 / 3.0]
    assert H.popularity_prior(z, -0.5).dtype == np.float32
    assert H.popularity_prior(z, -0.5).tolist() == [np.float32(-0.5 * v) for v in z.tolist()]
    with pytest.raises(ValueError):
        H.item_counts({"a": 0}, {"a": -1})


def test_set_popularity_on_a_hand_example():
    """Eight songs with counts 15 7 3 1 1 0 0 (and one without an entry): 27 plays in all."""
    from dcrecommend.nn.dcue import DCUE

    class Src:
        item_index = {"s%d" % i: i for i in range(8)}

    tr = DCUE.__new__(DCUE)
    tr._evals, tr._popularity, tr.train_data, tr._tracks_src = {}, None, None, None
    with pytest.raises(RuntimeError, match="set_popularity"):
        tr._popularity_arrays(Src)
    tr.set_popularity({"s0": 15, "s1": 7, "s2": 3, "s3": 1, "s4": 1, "s5": 0, "s6": 0})
    z, v, tail = tr._popularity_arrays(Src)
    assert z.tolist() == [1.0, 0.75, 0.5, 0.25, 0.25, 0.0, 0.0, 0.0]  # log2(1 + n) / log2(16)
    # sum (n + 1) = 16 + 8 + 4 + 2 + 2 + 1 + 1 + 1 = 35; -log2((n + 1) / 35)
    np.testing.assert_allclose(v, [np.log2(35 / 16), np.log2(35 / 8), np.log2(35 / 4), np.log2(35 / 2),
                                   np.log2(35 / 2), np.log2(35), np.log2(35), np.log2(35)], rtol=1e-15)
    # 0.8 * 27 = 21.6: 15 falls short, 15 + 7 = 22 holds it
    assert tail.tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    prior = tr._prior_kw(Src, -0.5, None)["prior"]
    assert prior.dtype == np.float32 and prior.tolist() == [-0.5, -0.375, -0.25, -0.125, -0.125, 0.0, 0.0, 0.0]
    assert tr._prior_kw(Src, -0.5, None)["prior"] is prior  # (kept: TopK caches its upload by identity)
    assert tr._prior_kw(Src, None, None) == {}
    with pytest.raises(ValueError, match="both"):
        tr._prior_kw(Src, 0.5, np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="finite"):
        tr._prior_kw(Src, float("nan"), None)
    # new counts forget the old arrays. 0.9 * 27 = 24.3: 22 falls short, 25 holds it
    tr.set_popularity({"s0": 15, "s1": 7, "s2": 3, "s3": 1, "s4": 1}, head_mass=0.9)
    assert tr._popularity_arrays(Src)[2].tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    tr.set_popularity({"s3": 1}, head_mass=0.5)
    assert tr._popularity_arrays(Src)[2].tolist() == [1, 1, 1, 0, 1, 1, 1, 1]


# ------------------------------------------------------------------------------- refusals
def _p():
    buf = (ctypes.c_uint8 * 64)()
    return ctypes.cast(buf, ctypes.c_void_p), buf


def _last_error():
    from dcrecommend import _native as nat
    return nat.lib().dcue_last_error().decode()


def _prior(**over):
    """dcue_topk_prior with never-dereferenced host addresses: every case returns before a device call."""
    from dcrecommend import _native as nat
    p, _keep = _p()
    a = dict(score=0, query_feat=p, n_query_rows=10, cand_feat=p, n_cand=1000, d=64, queries=p, n_queries=4,
             excl_ptr=p, excl_idx=p, cand_mask=p, cand_prior=p, k=10, query_batch=64, cand_split=0, ws=p, ws_bytes=0,
             out_idx=p, out_score=p, out_count=p, out_flags=p, stream=None)
    a.update(over)
    order = ("score", "query_feat", "n_query_rows", "cand_feat", "n_cand", "d", "queries", "n_queries", "excl_ptr",
             "excl_idx", "cand_mask", "cand_prior", "k", "query_batch", "cand_split", "ws", "ws_bytes", "out_idx",
             "out_score", "out_count", "out_flags", "stream")
    return nat.lib().dcue_topk_prior(*[a[n] for n in order])


@pytest.mark.parametrize("name", ["query_feat", "cand_feat", "queries", "ws", "out_idx", "out_score", "out_count",
                                  "out_flags"])
def test_prior_null_pointer_is_invalid(name):
    assert _prior(**{name: None}) == INVALID
    assert _last_error().startswith("dcue_topk_prior:")


@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(n_cand=0), dict(query_batch=0), dict(cand_split=-1),
                                  dict(excl_ptr=None), dict(excl_idx=None), dict(score=2), dict(score=-1),
                                  dict(n_queries=-1), dict(d=0)])
def test_prior_bad_argument_is_invalid(over):
    assert _prior(**over) == INVALID
    assert _last_error().startswith("dcue_topk_prior:")


def test_prior_unsupported_workspace_and_null_prior():
    assert _prior(d=257) == UNSUPPORTED and "256" in _last_error()
    assert _prior(n_cand=2 ** 31) == UNSUPPORTED
    assert _prior() == WORKSPACE and "workspace" in _last_error()  # valid arguments, 0 bytes
    assert _prior(score=1) == WORKSPACE
    assert _prior(cand_prior=None) == WORKSPACE  # a null prior is a valid call (dcue_topk_scored)
    assert _prior(n_queries=0) == OK


def _stats(**over):
    from dcrecommend import _native as nat
    p, _keep = _p()
    cut = (ctypes.c_int32 * 8)(*(list(over.pop("cutoffs", [1, 5, 10])) + [0] * 8)[:8])
    a = dict(idx=p, count=p, n_lists=4, k=10, item_value=p, item_tail=p, n_cand=1000,
             cutoffs=ctypes.cast(cut, ctypes.c_void_p), n_cutoffs=3, out_stats=p, out_flags=p, stream=None)
    a.update(over)
    order = ("idx", "count", "n_lists", "k", "item_value", "item_tail", "n_cand", "cutoffs", "n_cutoffs",
             "out_stats", "out_flags", "stream")
    return nat.lib().dcue_list_item_stats(*[a[n] for n in order])


@pytest.mark.parametrize("over", [dict(idx=None), dict(count=None), dict(cutoffs=None), dict(out_stats=None),
                                  dict(out_flags=None), dict(n_lists=-1), dict(k=0), dict(k=129), dict(n_cand=0),
                                  dict(n_cutoffs=0), dict(n_cutoffs=9), dict(cutoffs=[0, 5, 10]),
                                  dict(cutoffs=[1, 5, 11]), dict(cutoffs=[5, 5, 10]), dict(cutoffs=[5, 1, 10])])
def test_item_stats_bad_argument_is_invalid(over):
    if over.get("cutoffs", 0) is None:
        over = dict(over)
        del over["cutoffs"]
        from dcrecommend import _native as nat
        p, _keep = _p()
        assert nat.lib().dcue_list_item_stats(p, p, 4, 10, p, p, 1000, None, 3, p, p, None) == INVALID
    else:
        assert _stats(**over) == INVALID
    assert _last_error().startswith("dcue_list_item_stats:")


def test_item_stats_unsupported_and_empty():
    assert _stats(n_cand=2 ** 31) == UNSUPPORTED and "bound" in _last_error()
    assert _stats(n_lists=0) == OK  # nothing to do: no device call
    assert _stats(n_lists=0, item_value=None, item_tail=None) == OK


def test_item_stats_mean_refusals():
    from dcrecommend import _native as nat
    p, _keep = _p()
    fn = nat.lib().dcue_list_item_stats_mean
    for args in ((None, p, 4, 3, p, p), (p, None, 4, 3, p, p), (p, p, 4, 3, None, p), (p, p, 4, 3, p, None),
                 (p, p, -1, 3, p, p), (p, p, 4, 0, p, p), (p, p, 4, 9, p, p)):
        assert fn(*args, None) == INVALID
        assert _last_error().startswith("dcue_list_item_stats_mean:")


def _gini_ws(n_cand, m, n_lists):
    from dcrecommend import _native as nat
    n = ctypes.c_size_t(0)
    return nat.lib().dcue_exposure_gini_workspace_bytes(n_cand, m, n_lists, ctypes.byref(n)), n.value


def _gini(**over):
    from dcrecommend import _native as nat
    p, _keep = _p()
    a = dict(exposure=p, cand_mask=p, n_cand=1000, n_cutoffs=3, ws=p, ws_bytes=0, out_gini=p, out_total=p, stream=None)
    a.update(over)
    order = ("exposure", "cand_mask", "n_cand", "n_cutoffs", "ws", "ws_bytes", "out_gini", "out_total", "stream")
    return nat.lib().dcue_exposure_gini(*[a[n] for n in order])


def test_gini_workspace_bytes():
    from dcrecommend import _native as nat
    assert _gini_ws(200000, 3, 4096) == (OK, 64 + 3 * 4097 * 4)
    assert _gini_ws(1, 1, 0) == (OK, 64 + 4)
    assert _gini_ws(0, 3, 10)[0] == INVALID and _gini_ws(10, 0, 10)[0] == INVALID
    assert _gini_ws(10, 9, 10)[0] == INVALID and _gini_ws(10, 3, -1)[0] == INVALID
    assert nat.lib().dcue_exposure_gini_workspace_bytes(10, 3, 10, None) == INVALID
    assert _gini_ws(2 ** 31, 3, 10)[0] == UNSUPPORTED


def test_gini_refuses_shapes_that_could_reach_2_53():
    """n_cand * n_lists_max * 128 (DCUE_TOPK_MAX_K) must stay below 2^53."""
    n_cand = 2 ** 20
    edge = (2 ** 53 - 1) // 128 // n_cand  # 2^26 - 1
    assert _gini_ws(n_cand, 1, edge)[0] == OK
    assert _gini_ws(n_cand, 1, edge + 1)[0] == UNSUPPORTED and "2^53" in _last_error()
    assert _gini_ws(2 ** 31 - 100, 8, 2 ** 20)[0] == UNSUPPORTED
    assert _gini_ws(n_cand, 1, 2 ** 60)[0] == UNSUPPORTED
    # the call itself reads the bins back from ws_bytes
    ok_bytes = 64 + 4 * (edge + 1)
    assert _gini(n_cand=n_cand, n_cutoffs=1, ws_bytes=ok_bytes + 4) == UNSUPPORTED and "2^53" in _last_error()
    assert _gini(n_cand=n_cand, n_cutoffs=2, ws_bytes=2 * ok_bytes) == UNSUPPORTED


@pytest.mark.parametrize("over", [dict(exposure=None), dict(ws=None), dict(out_gini=None), dict(out_total=None),
                                  dict(n_cand=0), dict(n_cutoffs=0), dict(n_cutoffs=9)])
def test_gini_bad_argument_is_invalid(over):
    assert _gini(ws_bytes=1 << 20, **over) == INVALID
    assert _last_error().startswith("dcue_exposure_gini:")


def test_gini_workspace_too_small():
    assert _gini(ws_bytes=0) == WORKSPACE
    assert _gini(ws_bytes=64 + 3 * 4) == WORKSPACE and "bin" in _last_error()  # one bin per cutoff holds no count
    assert _gini(n_cand=2 ** 31, ws_bytes=1 << 20) == UNSUPPORTED


def test_python_layer_refuses_a_nonfinite_prior_before_upload():
    """TopK._prior_arg checks the host array: no device is touched (the TopK here has none)."""
    from dcrecommend.nn import rank
    tk = rank.TopK.__new__(rank.TopK)
    tk.n_cand, tk.device = 4, None
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="not finite at candidate 2"):
            tk._prior_arg(np.array([0.0, 1.0, bad, 0.0]))
    with pytest.raises(ValueError, match="4 candidates"):
        tk._prior_arg(np.zeros(5, np.float32))
    assert tk._prior_arg(None) is None
