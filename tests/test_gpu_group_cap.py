"""GPU tests of dcue_list_group_cap / dcue_list_group_stats / dcue_list_group_stats_mean (rank.GroupCap)
against the sequential restatement in group_reference.py. Lists are synthetic, written straight into device
tensors. Every comparison is exact: integers with ==, scores by their bits (nothing here rounds).

Shapes: pool at the lane-ownership and two-ballot boundaries (a lane owns positions l and l + 64),
n_lists at the four-waves-per-workgroup boundary and past one workgroup."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import group_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CAND = 300
POOLS = (1, 2, 63, 64, 65, 127, 128)
HUGE = 2 ** 31 - 1  # n_groups of the "huge" pattern: ids at n_groups - 1


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _gc():
    from dcrecommend.nn import rank
    return rank.GroupCap(DEV)


def _groups(pattern):
    """(group_of int32 [N_CAND], n_groups)"""
    i = np.arange(N_CAND)
    rs = np.random.RandomState(11)
    if pattern == "one":
        return np.zeros(N_CAND, np.int32), 1
    if pattern == "distinct":
        return i.astype(np.int32), N_CAND
    if pattern == "none":
        return np.full(N_CAND, -1, np.int32), 0
    if pattern == "alternating":
        return (i % 2).astype(np.int32), 2
    if pattern == "huge":
        return np.where(i % 3 == 0, HUGE - 1, np.where(i % 3 == 1, HUGE - 2, -1)).astype(np.int32), HUGE
    assert pattern == "mixed"  # a few groups of uneven size, some songs ungrouped
    return rs.choice(np.arange(-1, 7), N_CAND, p=[.1, .4, .2, .1, .05, .05, .05, .05]).astype(np.int32), 7


def _lists(rs, n, pool, repeats=False, hi=N_CAND):
    """idx [n, pool] over candidates below hi (no repeats within a list unless asked), score [n, pool] with a
    few special values."""
    idx = np.stack([rs.choice(hi, pool, replace=repeats) for _ in range(n)]).astype(np.int32)
    score = rs.randn(n, pool).astype(np.float32)
    score.reshape(-1)[::17] = np.float32(-0.0)
    score.reshape(-1)[5::41] = np.float32(np.inf)
    return idx, score


def _cap(idx, score, count, group_of, n_groups, cap, k_out, carry=None):
    c = None if carry is None else (_dev(carry[0], np.int32), _dev(carry[1], np.float32), _dev(carry[2], np.int32))
    out = _gc().cap_raw(_dev(idx, np.int32), _dev(score, np.float32), _dev(count, np.int32), _dev(group_of, np.int32),
                        n_groups, cap, k_out, carry=c)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want, what=""):
    assert np.array_equal(got[4], want[4]), (what, "flags", got[4], want[4])
    assert np.array_equal(got[2], want[2]), (what, "count", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "score bits")
    assert np.array_equal(got[3], want[3]), (what, "dropped", got[3], want[3])


def _counts(pool):
    return np.array([0, 1, pool - 1, pool, pool + 7], np.int32)  # (pool + 7: clamped to pool)


# ------------------------------------------------------------------------------------ the cap
@pytest.mark.parametrize("pattern", ["one", "distinct", "none", "alternating", "huge", "mixed"])
@pytest.mark.parametrize("pool", POOLS)
def test_cap_matches_the_sequential_walk(pool, pattern):
    group_of, n_groups = _groups(pattern)
    rs = np.random.RandomState(100 * pool + len(pattern))
    count = _counts(pool)
    idx, score = _lists(rs, len(count), pool)
    for cap in sorted({1, 2, pool}):
        for k_out in sorted({1, pool // 2 + 1, pool}):
            want = R.cap(idx, score, count, group_of, n_groups, cap, k_out)
            _same(_cap(idx, score, count, group_of, n_groups, cap, k_out), want, (cap, k_out))
            if cap == pool:  # composition: nothing can be dropped, the first k_out entries come back
                n = np.minimum(np.clip(count, 0, pool), k_out)
                for q in range(len(count)):
                    assert want[0][q, :n[q]].tolist() == idx[q, :n[q]].tolist() and want[3][q] == 0
                    assert np.array_equal(_bits(want[1][q, :n[q]]), _bits(score[q, :n[q]]))


@pytest.mark.parametrize("n_lists", [1, 3, 4, 5, 257])
def test_cap_over_workgroup_boundaries_with_repeated_candidates(n_lists):
    group_of, n_groups = _groups("mixed")
    for pool, cap, k_out in ((65, 2, 40), (128, 1, 128), (128, 3, 7)):
        rs = np.random.RandomState(n_lists + pool)
        idx, score = _lists(rs, n_lists, pool, repeats=True)  # an index named twice is two entries
        count = rs.randint(0, pool + 3, n_lists).astype(np.int32)
        count[-1] = pool
        _same(_cap(idx, score, count, group_of, n_groups, cap, k_out),
              R.cap(idx, score, count, group_of, n_groups, cap, k_out), (pool, cap, k_out))


@pytest.mark.parametrize("pattern", ["one", "alternating", "mixed", "huge", "none"])
@pytest.mark.parametrize("pool, k_out", [(1, 1), (2, 2), (63, 32), (64, 64), (65, 128), (127, 64), (128, 128), (128, 3)])
def test_cap_continues_a_carry(pool, k_out, pattern):
    """Carried entries come first, unchanged, and count toward their groups: 0, 1, k_out - 1 and k_out of
    them (a full carry passes through), one count above k_out (clamped), one carry that already
    saturates group 0 / the first group of the pattern."""
    group_of, n_groups = _groups(pattern)
    rs = np.random.RandomState(7 * pool + k_out)
    kcs = np.array([0, 1, k_out - 1, k_out, k_out + 3, min(2, k_out)], np.int32)
    n = len(kcs)
    idx, score = _lists(rs, n, pool)
    count = np.full(n, pool, np.int32)
    cidx, cscore = _lists(rs, n, k_out)
    first = int(group_of[idx[n - 1, 0]])
    if first >= 0:  # the last list's carry: entries of the group its pool starts with
        cidx[n - 1, :] = np.resize(np.flatnonzero(group_of == first), k_out)
    for cap in (1, 2, pool):
        want = R.cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs))
        got = _cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs))
        _same(got, want, cap)
        for q, kc in enumerate(np.minimum(kcs, k_out)):
            assert got[0][q, :kc].tolist() == cidx[q, :kc].tolist()
            assert np.array_equal(_bits(got[1][q, :kc]), _bits(cscore[q, :kc]))
        assert got[2][3] == k_out and got[2][4] == k_out and got[4][3] == 0  # the full carries
        if first >= 0 and cap <= min(2, k_out):  # the saturated group's pool entries are all dropped
            kept = got[0][n - 1, min(2, k_out):got[2][n - 1]]
            assert not np.any(group_of[kept] == first)


@pytest.mark.parametrize("where, value, flag", [
    ("pool", -1, R.BAD_INDEX), ("pool", N_CAND, R.BAD_INDEX), ("carry", -1, R.BAD_INDEX), ("carry", N_CAND, R.BAD_INDEX),
    ("group", -2, R.BAD_GROUP), ("group", 7, R.BAD_GROUP), ("carry group", -2, R.BAD_GROUP)])
def test_cap_flags_leave_the_other_lists_alone(where, value, flag):
    group_of, n_groups = _groups("mixed")
    group_of = group_of.copy()
    rs = np.random.RandomState(5)
    pool, k_out, cap, n, bad = 100, 60, 2, 6, 2
    idx, score = _lists(rs, n, pool, hi=280)
    count = np.array([pool, 70, 90, 64, 65, 1], np.int32)
    cidx, cscore = _lists(rs, n, k_out, hi=280)
    kcs = np.array([3, 0, 5, 1, 0, 2], np.int32)
    idx[bad, 70], cidx[bad, 0] = 290, 291  # candidates that only the list that goes bad names
    clean = _cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs))
    assert not (clean[4] & ~R.SHORT).any()
    if where == "pool":
        idx[bad, 89] = value  # the last position the count reaches
    elif where == "carry":
        cidx[bad, 4] = value
    else:
        group_of[290 if where == "group" else 291] = value
    got = _cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs))
    _same(got, R.cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs)))
    assert got[4][bad] == flag and got[2][bad] == 0 and got[3][bad] == 0
    assert (got[0][bad] == -1).all() and np.isneginf(got[1][bad]).all()
    keep = np.arange(n) != bad
    for g, c in zip(got, clean):
        assert np.array_equal(g[keep].view(np.uint32) if g.dtype == np.float32 else g[keep],
                              c[keep].view(np.uint32) if c.dtype == np.float32 else c[keep])
    # an entry past the count is never read, whatever it holds
    idx2 = idx.copy()
    idx2[0, :] = np.where(np.arange(pool) >= 50, 2 ** 31 - 1, idx2[0])
    count2 = count.copy()
    count2[0] = 50
    _same(_cap(idx2, score, count2, group_of, n_groups, cap, k_out),
          R.cap(idx2, score, count2, group_of, n_groups, cap, k_out))


def test_cap_does_not_depend_on_the_launch():
    group_of, n_groups = _groups("mixed")
    rs = np.random.RandomState(9)
    pool, k_out, cap, n = 128, 90, 2, 13
    idx, score = _lists(rs, n, pool, repeats=True)
    count = rs.randint(60, pool + 1, n).astype(np.int32)
    cidx, cscore = _lists(rs, n, k_out)
    kcs = rs.randint(0, 6, n).astype(np.int32)
    whole = _cap(idx, score, count, group_of, n_groups, cap, k_out, carry=(cidx, cscore, kcs))
    order = rs.permutation(n)
    mixed = _cap(idx[order], score[order], count[order], group_of, n_groups, cap, k_out,
                 carry=(cidx[order], cscore[order], kcs[order]))
    for q in range(n):
        alone = _cap(idx[q:q + 1], score[q:q + 1], count[q:q + 1], group_of, n_groups, cap, k_out,
                     carry=(cidx[q:q + 1], cscore[q:q + 1], kcs[q:q + 1]))
        at = int(np.flatnonzero(order == q)[0])
        for w, a, s in zip(whole, alone, mixed):
            assert np.array_equal(_bits(w[q]) if w.dtype == np.float32 else w[q], _bits(a[0]) if a.dtype == np.float32 else a[0])
            assert np.array_equal(_bits(w[q]) if w.dtype == np.float32 else w[q], _bits(s[at]) if s.dtype == np.float32 else s[at])


# ------------------------------------------------------------------------------------ the statistics
CUTOFFS = ((1,), (1, 2, 64, 65, 128), (1, 2, 3, 63, 64, 65, 127, 128))


def _stats(idx, count, group_of, n_groups, ks, exposure=None):
    st, flags = _gc().stats_raw(_dev(idx, np.int32), _dev(count, np.int32), _dev(group_of, np.int32), n_groups, ks,
                                exposure=exposure)
    return st.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("pattern", ["one", "distinct", "none", "alternating", "mixed"])
@pytest.mark.parametrize("ks", CUTOFFS)
def test_stats_and_exposure_match_the_reference(ks, pattern):
    group_of, n_groups = _groups(pattern)
    rs = np.random.RandomState(len(ks) + len(pattern))
    k = max(ks)
    for n in (1, 5, 257):
        idx, _ = _lists(rs, n, k, repeats=True)
        count = rs.randint(0, k + 4, n).astype(np.int32)
        count[:min(n, 4)] = [0, 1, k - 1 if k > 1 else 1, k][:min(n, 4)]
        want_exp = np.zeros((len(ks), n_groups), np.int64)
        want = R.stats(idx, count, group_of, n_groups, ks, want_exp)
        exposure = _gc().new_exposure(len(ks), n_groups)
        got = _stats(idx, count, group_of, n_groups, ks, exposure)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (n, ks)
        assert np.array_equal(exposure.cpu().numpy(), want_exp)
        assert np.array_equal(_stats(idx, count, group_of, n_groups, ks)[0], want[0])  # without the table


def test_stats_means_are_the_same_bits_however_batched():
    """Means and coverage equal numpy's with == under three batchings into the stats buffer; a flagged
    list (a bad index, a bad group) is left out of the means and of the exposure."""
    group_of, n_groups = _groups("mixed")
    group_of = group_of.copy()
    rs = np.random.RandomState(21)
    ks, k, n = (1, 2, 64, 65, 128), 128, 301
    idx, _ = _lists(rs, n, k, hi=280)
    count = rs.randint(0, k + 1, n).astype(np.int32)
    idx[7, 3], count[7] = N_CAND, 10  # BAD_INDEX
    idx[100, 0], group_of[290], count[100] = 290, 7, 5  # BAD_GROUP, of a candidate no other list names
    present = (rs.rand(n_groups) < 0.8).astype(np.uint8)
    want_exp = np.zeros((len(ks), n_groups), np.int64)
    want_st, want_flags = R.stats(idx, count, group_of, n_groups, ks, want_exp)
    assert want_flags[7] == R.BAD_INDEX and want_flags[100] == R.BAD_GROUP
    mean, cov, n_eval = R.stats_mean(want_st, want_flags, want_exp, present)
    assert n_eval == n - 2
    gc = _gc()
    idx_d, count_d, g_d = _dev(idx, np.int32), _dev(count, np.int32), _dev(group_of, np.int32)
    cut = (ctypes.c_int32 * len(ks))(*ks)
    for batch in (n, 64, 7):
        st = torch.zeros((n, len(ks), 2), dtype=torch.int32, device=DEV)
        flags = torch.zeros(n, dtype=torch.int32, device=DEV)
        exposure = gc.new_exposure(len(ks), n_groups)
        for q0 in range(0, n, batch):
            gc._stats_into(idx_d[q0:q0 + batch], count_d[q0:q0 + batch], g_d, n_groups, list(ks), cut, st[q0:],
                           flags[q0:], exposure)
        assert np.array_equal(st.cpu().numpy(), want_st) and np.array_equal(flags.cpu().numpy(), want_flags)
        assert np.array_equal(exposure.cpu().numpy(), want_exp)
        got = gc.mean_raw(st, flags, exposure, _dev(present, np.uint8))
        assert np.array_equal(got[0].cpu().numpy().view(np.uint64), mean.view(np.uint64)), batch
        assert np.array_equal(got[1].cpu().numpy().view(np.uint64), cov.view(np.uint64)), batch
        assert int(got[2].cpu()[0]) == n_eval
    got = gc.mean_raw(st, flags)  # without the table: no coverage
    assert got[1] is None and np.array_equal(got[0].cpu().numpy().view(np.uint64), mean.view(np.uint64))
    none = gc.mean_raw(st[:0], flags[:0])
    assert int(none[2].cpu()[0]) == 0 and not none[0].cpu().numpy().any()
