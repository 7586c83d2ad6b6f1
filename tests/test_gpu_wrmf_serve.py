"""GPU tests of the WRMF / DCBR serving path: the inner-product top-K
(dcue_topk_scored, rank.TopK(score="dot")), the sparse objective (dcue_wrmf_objective), the closed-form
fold-in and the WRMF / DCBR entry points over them.

Exact lists use integer factors: entries in {-3..3}, candidate rows scaled by 2^e, e in {-2..3}. Every
product is a multiple of 2^-2 of size at most 72, so a sum of d <= 256 of them is a multiple of 2^-2
below 2^24 (in units of 2^-2: 256 * 72 * 4 < 2^17): exact in fp32 in any summation order, and idx,
count and the bits of score must equal the fp64 reference's, tie order included.

Gaussian lists are held to tol_q = 1.01 d 2^-24 |q| max_c |c|, the standard forward bound of a d-term
fp32 dot product (gamma_d |q| |c|, gamma_d = d u / (1 - d u), u = 2^-24; 1.01 covers the denominator):
derived, not measured.

The objective is held to 1e-9 relative against the dense fp64 oracle: at most 3e4 summed terms
(12k pairs, d^2 Gram entries) x 2^-53 x the amplification A = (sum |observed terms| +
sum |G_X o G_Y| + regulariser) / L, which the test computes in numpy and requires to be <= 100 (the
largest at these shapes after ALS iterations is about 70): 3e4 * 1.1e-16 * 100 = 3.3e-10.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import topk_metrics_reference as M
import topk_reference as T
import wrmf_serve_reference as R
from oracle import wrmf_oracle as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 0.05


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _dots(qf, cand, queries):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(qf, np.float64)[np.asarray(queries)] @ np.asarray(cand, np.float64).T


def _excl_rows(rs, n_rows, n_cand, max_excl):
    ptr, idx = [0], []
    for _ in range(n_rows):
        n = min(rs.randint(0, max_excl + 1), n_cand)
        idx.append(np.sort(rs.choice(n_cand, n, replace=False)))
        ptr.append(ptr[-1] + n)
    return np.array(ptr, np.int64), np.concatenate(idx).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _int_case(seed, n_cand, d, n_rows=130, n_queries=150, negative=False):
    """Integer factors (module docstring) with 5 % duplicated rows and 3 zero rows, exclusion rows of
    0..150 sorted items, an 80 % mask, queries with repeats, and the fp64 dot products. negative: every
    query entry in {1..3} and every candidate entry in -{1..3} 2^e (no zero rows): every score < 0."""
    rs = np.random.RandomState(seed)
    scale = 2.0 ** rs.randint(-2, 4, (n_cand, 1))
    if negative:
        cand = (-rs.randint(1, 4, (n_cand, d)) * scale).astype(np.float32)
        qf = rs.randint(1, 4, (n_rows, d)).astype(np.float32)
    else:
        cand = (rs.randint(-3, 4, (n_cand, d)) * scale).astype(np.float32)
        qf = rs.randint(-3, 4, (n_rows, d)).astype(np.float32)
    dup = rs.choice(n_cand, n_cand // 20, replace=False)
    cand[dup] = cand[rs.choice(n_cand, len(dup))]
    if not negative:
        cand[rs.choice(n_cand, 3, replace=False)] = 0.0
    ptr, idx = _excl_rows(rs, n_rows, n_cand, 150)
    c = dict(qf=qf, cand=cand, ptr=ptr, idx=idx, mask=(rs.rand(n_cand) < 0.8).astype(np.uint8),
             queries=rs.randint(0, n_rows, n_queries))
    c["s64"] = _dots(qf, cand, c["queries"])
    return c


@functools.lru_cache(maxsize=None)
def _gauss_case(d, n_cand=4099, n_rows=65):
    """Gaussian queries; candidates Gaussian x exp(N(0, 1)) per row (log-normal norms); no exclusion."""
    rs = np.random.RandomState(900 + d)
    cand = (rs.randn(n_cand, d) * np.exp(rs.randn(n_cand, 1))).astype(np.float32)
    qf = rs.randn(n_rows, d).astype(np.float32)
    c = dict(qf=qf, cand=cand, ptr=None, idx=None, mask=None, queries=np.arange(n_rows))
    c["s64"] = _dots(qf, cand, c["queries"])
    return c


def _topk(c, score, excl=True, mask=True):
    from dcrecommend.nn import rank
    return rank.TopK(c["ptr"] if excl else None, c["idx"] if excl else None, c["mask"] if mask else None, DEV,
                     n_cand=len(c["cand"]), score=score)


def _run(c, k, score="dot", query_batch=None, cand_split=0, excl=True, mask=True, raw=False):
    tk = _topk(c, score, excl, mask)
    fn = tk.topk_raw if raw else tk.topk
    return fn(torch.from_numpy(c["qf"]).to(DEV), torch.from_numpy(c["cand"]).to(DEV), c["queries"], k,
              query_batch=query_batch, cand_split=cand_split)


def _assert_exact(got, c, k, excl=True, mask=True):
    want = T.topk(None, None, c["queries"], k, c["ptr"] if excl else None, c["idx"] if excl else None,
                  c["mask"] if mask else None, scores=c["s64"])
    idx, score, count = got
    assert idx.dtype == np.int64 and score.dtype == np.float32 and count.dtype == np.int32
    assert np.array_equal(count, want[2])
    assert np.array_equal(idx, want[0])
    assert np.array_equal(_bits(score), _bits(want[1] + 0.0))


# ------------------------------------------------------------------------------------- exact dot lists
@pytest.mark.parametrize("n_cand", [63, 64, 65, 2500])
@pytest.mark.parametrize("d", [1, 7, 16, 100, 130, 256])
def test_dot_integer_exact(d, n_cand):
    c = _int_case(1000 + 7 * d + n_cand, n_cand, d)
    assert np.abs(c["s64"]).max() < 2 ** 22 and np.all(c["s64"] * 4 == np.round(c["s64"] * 4))
    for k in (1, 33, 128):
        _assert_exact(_run(c, k), c, k)


def test_dot_every_score_negative():
    """Negative scores' keys sort above the empty-slot key: the lists are full and ordered."""
    c = _int_case(31, 2500, 100, negative=True)
    assert c["s64"].max() < 0
    for k in (1, 33, 128):
        got = _run(c, k)
        assert np.all(got[2] == k) and np.all(got[1] < 0)
        _assert_exact(got, c, k)


def test_dot_fewer_eligible_than_k_pads():
    c = dict(_int_case(32, 2500, 100))
    mask = np.zeros(2500, np.uint8)
    mask[[3, 64, 1000, 2436, 2499]] = 1
    c["mask"] = mask
    got = _run(c, 33)
    assert np.all(got[2] <= 5) and got[2].max() > 0
    assert np.all(got[0][:, 5:] == -1) and np.all(np.isneginf(got[1][:, 5:]))
    _assert_exact(got, c, 33)


# ------------------------------------------------------------------------------------- tolerant dot lists
@pytest.mark.parametrize("d", [100, 128, 256])
def test_dot_gaussian_vs_fp64(d):
    k = 33
    c = _gauss_case(d)
    s64 = c["s64"]
    qn = np.sqrt((c["qf"].astype(np.float64) ** 2).sum(1))
    cmax = np.sqrt((c["cand"].astype(np.float64) ** 2).sum(1)).max()
    tol = 1.01 * d * 2.0 ** -24 * qn * cmax
    # the band must not be so wide that it lets anything pass: few candidates near the k-th score
    kth = np.sort(s64, axis=1)[:, ::-1][:, k - 1]
    near = (np.abs(s64 - kth[:, None]) <= 2 * tol[:, None]).sum(1)
    print("d=%d: candidates within 2 tol of the k-th score, max over queries: %d" % (d, near.max()))
    assert near.max() <= 8
    idx, score, count = _run(c, k, excl=False, mask=False)
    ok = np.ones(s64.shape[1], bool)
    for i in range(len(c["queries"])):
        T.check_tolerant(idx[i], score[i], int(count[i]), s64[i], ok, k, tol[i])
    # the cosine list of the same inputs is another list: this test cannot pass on the cosine path
    cidx = _run(c, k, score="cosine", excl=False, mask=False)[0]
    shared = sum(len(np.intersect1d(idx[i], cidx[i])) for i in range(len(idx)))
    print("d=%d: dot and cosine lists share %.1f %% of their entries" % (d, 100.0 * shared / idx.size))
    assert shared < 0.5 * idx.size


# ------------------------------------------------------------------------------------- tilings
@pytest.mark.parametrize("kind,d,k", [("int", 100, 33), ("gauss", 128, 33)])
def test_dot_deterministic_across_tilings(kind, d, k):
    c = _int_case(1000 + 7 * d + 2500, 2500, d) if kind == "int" else _gauss_case(d)
    excl = kind == "int"
    first = None
    for split in (1, 2, 5, 0):
        for qb in (16, 64, 1000):
            idx, score, count = _run(c, k, query_batch=qb, cand_split=split, excl=excl, mask=excl)
            if first is None:
                first = (idx, _bits(score), count)
                continue
            assert np.array_equal(idx, first[0]), (split, qb)
            assert np.array_equal(_bits(score), first[1]), (split, qb)
            assert np.array_equal(count, first[2]), (split, qb)


# ------------------------------------------------------------------------------------- cosine unchanged
def _lattice(rs, n, d):
    x = np.zeros((n, d), np.float32)
    for r in range(n):
        x[r, rs.choice(d, 16, replace=False)] = rs.choice(np.array([-1.0, 1.0], np.float32), 16)
    return x


def _library_call(score, c, k):
    """dcue_topk (score None) or dcue_topk_scored straight from the library: (idx, score bits, count, flags)."""
    from dcrecommend import _native as nat
    qf, cand = torch.from_numpy(c["qf"]).to(DEV), torch.from_numpy(c["cand"]).to(DEV)
    q = torch.from_numpy(c["queries"].astype(np.int32)).to(DEV)
    ptr, eidx = torch.from_numpy(c["ptr"]).to(DEV), torch.from_numpy(c["idx"]).to(DEV)
    mask = torch.from_numpy(c["mask"]).to(DEV)
    nq, n_cand, d = int(q.numel()), cand.shape[0], cand.shape[1]
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib().dcue_topk_workspace_bytes(n_cand, d, nq, k, 0, ctypes.byref(nbytes)), "workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    idx = torch.full((nq, k), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((nq, k), 7.0, dtype=torch.float32, device=DEV)
    count = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    args = (nat.ptr(qf), qf.shape[0], nat.ptr(cand), n_cand, d, nat.ptr(q), nq, nat.ptr(ptr), nat.ptr(eidx),
            nat.ptr(mask), k, nq, 0, nat.ptr(ws), ws.numel(), nat.ptr(idx), nat.ptr(sc), nat.ptr(count),
            nat.ptr(flags), nat.stream_handle())
    if score is None:
        nat.check(nat.lib().dcue_topk(*args), "dcue_topk")
    else:
        nat.check(nat.lib().dcue_topk_scored(score, *args), "dcue_topk_scored")
    return idx.cpu().numpy(), _bits(sc.cpu().numpy()), count.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("lattice", [False, True])
def test_cosine_through_scored_is_dcue_topk(lattice):
    from dcrecommend import _native as nat
    rs = np.random.RandomState(41 + lattice)
    n_rows, n_cand, d, k = 130, 2500, 100, 50
    c = dict(qf=_lattice(rs, n_rows, d) if lattice else rs.randn(n_rows, d).astype(np.float32),
             cand=_lattice(rs, n_cand, d) if lattice else rs.randn(n_cand, d).astype(np.float32),
             mask=(rs.rand(n_cand) < 0.8).astype(np.uint8), queries=rs.randint(0, n_rows, 150))
    c["ptr"], c["idx"] = _excl_rows(rs, n_rows, n_cand, 150)
    a, b = _library_call(None, c, k), _library_call(nat.SCORE_COSINE, c, k)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    want = T.topk(c["qf"], c["cand"], c["queries"], k, c["ptr"], c["idx"], c["mask"])
    assert np.array_equal(a[2], want[2])
    if lattice:  # (every cosine a multiple of 1/16: exact)
        assert np.array_equal(a[0], want[0])
    # and the dot call is another computation on the same inputs (norms differ on the Gaussian rows)
    dot = _library_call(nat.SCORE_DOT, c, k)
    assert np.array_equal(dot[2], a[2]) and not np.array_equal(dot[1], a[1])


# ------------------------------------------------------------------------------------- non-finite
def test_dot_overflow_and_nan():
    rs = np.random.RandomState(5)
    cand = rs.randn(200, 32).astype(np.float32)
    cand[5] = 1e30
    cand[9] = np.nan
    qf = rs.randn(4, 32).astype(np.float32)
    qf[0] = 1e30
    c = dict(qf=qf, cand=cand, ptr=None, idx=None, mask=None, queries=np.array([0, 1, 2, 0]))
    idx, score, count, flags = [x.cpu().numpy() for x in _run(c, 10, excl=False, mask=False, raw=True)]
    assert np.all(flags & 2), "an eligible candidate's score is NaN (row 9) for every query"
    assert not np.any(idx == 9), "a NaN is never returned"
    assert np.all(count == 10)
    for i in (0, 3):  # 32 products of 1e60 overflow to +inf: first, as an ordinary value
        assert idx[i, 0] == 5 and np.isposinf(score[i, 0]) and np.all(np.isfinite(score[i, 1:]))
    # the ordinary queries: row 5 scores 1e30 * sum(q), first or nowhere; the rest as usual
    s64 = _dots(qf, cand, c["queries"])
    ok = np.ones(200, bool)
    ok[[5, 9]] = False
    cmax = np.sqrt((cand[ok].astype(np.float64) ** 2).sum(1)).max()
    for i in (1, 2):
        assert np.all(np.isfinite(score[i]))
        assert (idx[i, 0] == 5) == (s64[i, 5] > 0) and not np.any(idx[i, 1:] == 5)
        rest = slice(1, None) if idx[i, 0] == 5 else slice(None)
        tol = 1.01 * 32 * 2.0 ** -24 * np.sqrt((qf[c["queries"][i]].astype(np.float64) ** 2).sum()) * cmax
        n = len(idx[i, rest])
        T.check_tolerant(idx[i, rest].astype(np.int64), score[i, rest], n, s64[i], ok, n, tol)
    with pytest.raises(ValueError, match="overflowed"):
        _run(c, 10, excl=False, mask=False)
    # without the NaN row and the overflowing query nothing is flagged
    c2 = dict(c, cand=np.delete(cand, 9, axis=0), queries=np.array([1, 2]))
    assert not np.any(_run(c2, 10, excl=False, mask=False, raw=True)[3].cpu().numpy() & 2)


def test_score_argument_is_checked():
    from dcrecommend.nn import rank
    with pytest.raises(ValueError, match="score"):
        rank.TopK(None, None, None, DEV, n_cand=10, score="euclid")


# ------------------------------------------------------------------------------------- the objective
def _model(p, alpha, X=None, Y=None, iterations=0):
    """A WRMF over problem p with the given factors in place (no fit)."""
    from dcrecommend.dcbr import WRMF, device_csr
    m = WRMF(factors=p["d"], regularization=LAM, alpha=alpha, iterations=iterations, device=DEV)
    r, c = torch.as_tensor(p["rows"], device=DEV), torch.as_tensor(p["cols"], device=DEV)
    v = None if p["values"] is None else torch.as_tensor(p["values"], device=DEV)
    m.by_user = device_csr(r, c, v, p["n_users"])
    m.by_item = device_csr(c, r, v, p["n_items"])
    m.init_factors(p["n_users"], p["n_items"])
    m.user_factors.copy_(torch.from_numpy(p["X"] if X is None else X))
    m.item_factors.copy_(torch.from_numpy(p["Y"] if Y is None else Y))
    return m


OBJ_CASES = {"300x500": (300, 500, 100, True, {}), "257x131": (257, 131, 128, False, {}),
             "40x33": (40, 33, 7, True, {}), "1x1": (1, 1, 1, True, {}),
             "empty-user": (40, 33, 7, True, dict(empty_user=3)), "empty-item": (257, 131, 128, False, dict(empty_item=5))}


@functools.lru_cache(maxsize=None)
def _obj_problem(name):
    nu, ni, d, vals, kw = OBJ_CASES[name]
    return R.problem(11 + nu, nu, ni, d, vals, **kw)


@functools.lru_cache(maxsize=None)
def _obj_factors(name, alpha, iters):
    p = _obj_problem(name)
    return (p["X"], p["Y"]) if iters == 0 else R.als_iterations(p, alpha, LAM, iters)


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("alpha", [1.0, 40.0])
@pytest.mark.parametrize("name", sorted(OBJ_CASES))
def test_objective_against_dense_oracle(name, alpha, iters):
    p = _obj_problem(name)
    X, Y = _obj_factors(name, alpha, iters)
    want = W.objective(X, Y, p["rows"], p["cols"], p["values"], alpha, LAM)
    terms = R.objective_terms(X, Y, p["rows"], p["cols"], p["values"], alpha, LAM)
    A = R.amplification(X, Y, p["rows"], p["cols"], p["values"], alpha, LAM)
    assert A <= 100, A
    m = _model(p, alpha, X, Y)
    got = m.objective_terms()
    print("%s alpha=%g iters=%d: A %.1f, L %.17g, oracle %.17g, rel %.2e"
          % (name, alpha, iters, A, got[0], want, abs(got[0] - want) / abs(want)))
    assert abs(got[0] - want) <= 1e-9 * abs(want)
    for g, t in zip(got, terms):
        assert abs(g - t) <= 1e-9 * abs(want), (got, terms)
    assert m.objective() == got[0] and m.objective_terms() == got  # two calls, the same bits
    assert abs(m.loss() - want) <= 1e-9 * abs(want)


def test_objective_without_pairs_and_bad_index():
    from dcrecommend.dcbr import device_csr
    p = dict(_obj_problem("40x33"))
    p["rows"], p["cols"], p["values"] = p["rows"][:0], p["cols"][:0], None
    got = _model(p, 40.0).objective_terms()
    want = R.objective_terms(p["X"], p["Y"], p["rows"], p["cols"], None, 40.0, LAM)
    assert got[1] == 0.0 and want[1] == 0.0
    for g, t in zip(got, want):
        assert abs(g - t) <= 1e-9 * abs(want[0])
    # an item index past the table is not dereferenced: the observed term is NaN
    p = _obj_problem("40x33")
    m = _model(p, 40.0)
    cols = torch.as_tensor(p["cols"], device=DEV).clone()
    cols[7] = p["n_items"] + 1000
    m.by_user = device_csr(torch.as_tensor(p["rows"], device=DEV), cols, None, p["n_users"])
    got = m.objective_terms()
    assert np.isnan(got[0]) and np.isnan(got[1]) and np.isfinite(got[2]) and np.isfinite(got[3])


def test_fit_tracks_the_objective():
    from dcrecommend.dcbr import WRMF
    p = _obj_problem("300x500")
    m = WRMF(factors=100, regularization=LAM, alpha=40.0, iterations=4, seed=2, device=DEV)
    m.fit(p["rows"], p["cols"], p["values"], n_users=300, n_items=500, track_objective=True)
    h = m.objective_history
    print("objective history:", h)
    assert len(h) == 4
    for a, b in zip(h, h[1:]):
        assert b <= a * (1 + 1e-9)
    assert abs(h[-1] - m.loss()) <= 1e-9 * abs(m.loss())


def test_fit_tol_stops_early():
    """An oracle ALS run of this problem (numpy, fp64) lowers L by less than 5 % from its 5th
    iteration on."""
    from dcrecommend.dcbr import WRMF
    p = _obj_problem("40x33")
    m = WRMF(factors=7, regularization=LAM, alpha=40.0, iterations=30, seed=2, device=DEV)
    m.fit(p["rows"], p["cols"], p["values"], n_users=40, n_items=33, tol=0.05)
    h = m.objective_history
    assert 2 <= len(h) < 30
    assert h[-2] - h[-1] < 0.05 * abs(h[-2])
    assert all(a - b >= 0.05 * abs(a) for a, b in zip(h[:-2], h[1:-1]))


def test_default_fit_is_unchanged():
    """fit() with the defaults: the factors of the plain sweep loop, bit for bit, and no objective call."""
    from dcrecommend.dcbr import WRMF
    p = _obj_problem("257x131")
    a = WRMF(factors=128, regularization=LAM, alpha=40.0, iterations=2, seed=4, device=DEV)
    calls = []
    a.objective = lambda: calls.append(1) or 0.0
    a.fit(p["rows"], p["cols"], p["values"], n_users=257, n_items=131)
    assert not calls and not getattr(a, "objective_history", [])
    b = _model(p, 40.0, iterations=2)
    b.seed = 4
    b.init_factors(257, 131)
    for _ in range(2):
        b.half_step(b.user_factors, b.item_factors, b.by_user)
        b.half_step(b.item_factors, b.user_factors, b.by_item)
    assert torch.equal(a.user_factors, b.user_factors) and torch.equal(a.item_factors, b.item_factors)


# ------------------------------------------------------------------------------------- fold-in
@pytest.mark.parametrize("with_values", [False, True])
@pytest.mark.parametrize("d", [7, 100, 128])
def test_fold_in_against_oracle(d, with_values):
    rs = np.random.RandomState(60 + d)
    n_items = 131
    p = R.problem(70 + d, 50, n_items, d, with_values)
    p["Y"] = (rs.randn(n_items, d) * 0.3).astype(np.float32)
    m = _model(p, 3.0)
    before = m.user_factors.clone()
    sizes = [0, 1, 31, 32, 33, 70]
    hist = [rs.choice(n_items, n, replace=False) for n in sizes]
    vals = [rs.randint(1, 21, n).astype(np.float32) for n in sizes] if with_values else None
    got = m.fold_in(hist, vals)
    assert got.is_cuda and tuple(got.shape) == (len(sizes), d)
    got = got.cpu().numpy().astype(np.float64)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    ref = W.half_step(p["Y"], ptr, np.concatenate(hist), None if vals is None else np.concatenate(vals), 3.0, LAM)
    scale = np.abs(ref).max()
    for r, n in enumerate(sizes):
        err = np.abs(got[r] - ref[r]).max() / scale
        assert err <= 1e-4, "history of %d items: %.3e of max" % (n, err)
    assert np.all(got[0] == 0.0)
    assert torch.equal(m.user_factors, before)
    with pytest.raises(ValueError):
        m.fold_in([[0, n_items]])
    with pytest.raises(ValueError):
        m.fold_in([[-1]])
    assert tuple(m.fold_in([]).shape) == (0, d)


@pytest.mark.parametrize("with_values", [False, True])
def test_fold_in_of_fitted_rows_is_the_half_step(with_values):
    p = R.problem(81, 300, 500, 100, with_values, empty_user=3)
    m = _model(p, 40.0)
    want = m.user_factors.clone()
    m.half_step(want, m.item_factors, m.by_user)
    indptr, indices, values = [None if t is None else t.cpu().numpy() for t in m.by_user]
    users = [0, 3, 17, 299, 150, 17]
    hist = [indices[indptr[u]:indptr[u + 1]] for u in users]
    vals = [values[indptr[u]:indptr[u + 1]] for u in users] if with_values else None
    got = m.fold_in(hist, vals)
    assert torch.equal(got, want[users])
    assert torch.all(got[1] == 0)


# ------------------------------------------------------------------------------------- the entry points
@functools.lru_cache(maxsize=None)
def _served():
    """A 300 x 500, d = 100 model with one oracle ALS iteration's factors."""
    p = _obj_problem("300x500")
    X, Y = _obj_factors("300x500", 40.0, 2)
    return p, X, Y


def _tol(X, Y, rows, d):
    return 1.01 * d * 2.0 ** -24 * np.sqrt((X[rows].astype(np.float64) ** 2).sum(1)) * \
        np.sqrt((Y.astype(np.float64) ** 2).sum(1)).max()


def test_recommend_excludes_the_seen_items():
    p, X, Y = _served()
    m = _model(p, 40.0, X, Y)
    users = np.array([0, 7, 299, 7, 120])
    k = 20
    ptr, idx, _ = W.csr(p["rows"], p["cols"], None, 300)
    idx = idx.astype(np.int32)  # (problem() lists each user's items in ascending order)
    s64 = _dots(X, Y, users)
    tol = _tol(X, Y, users, 100)
    for exclude in (True, False):
        got = m.recommend(users, k, exclude_seen=exclude)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[0].shape == (5, k)
        for i, u in enumerate(users):
            ok = T.eligible(s64[i], int(u), ptr if exclude else None, idx, None)
            T.check_tolerant(got[0][i], got[1][i], int(got[2][i]), s64[i], ok, k, tol[i])
            seen = idx[ptr[u]:ptr[u + 1]]
            if exclude:
                assert not len(np.intersect1d(got[0][i], seen))
    # an unsorted interaction list with a repeated pair excludes the same items
    order = np.random.RandomState(3).permutation(len(p["rows"]))
    rows = np.concatenate([p["rows"][order], p["rows"][:5]])
    cols = np.concatenate([p["cols"][order], p["cols"][:5]])
    q = dict(p, rows=rows, cols=cols, values=None)
    m2 = _model(q, 40.0, X, Y)
    a, b = m.recommend(users, k), m2.recommend(users, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    # a candidate mask
    mask = (np.random.RandomState(4).rand(500) < 0.5).astype(np.uint8)
    got = m.recommend(users, k, cand_mask=mask)
    assert np.all(mask[got[0][got[0] >= 0]] == 1)


def test_recommend_for_excludes_the_history():
    p, X, Y = _served()
    m = _model(p, 40.0, X, Y)
    rs = np.random.RandomState(8)
    # the first history is a fitted user's own row: the factors score its items near 1 and the rest
    # near 0, so without the exclusion they fill the list and the exclusion is seen to act
    hist = [p["cols"][p["rows"] == 0].tolist()] + [rs.choice(500, n, replace=False).tolist() for n in (1, 0, 70)]
    k = 25
    feat = m.fold_in(hist).cpu().numpy()
    s64 = feat.astype(np.float64) @ Y.astype(np.float64).T
    tol = _tol(feat, Y, np.arange(4), 100)
    got = m.recommend_for(hist, k)
    free = m.recommend_for(hist, k, exclude_history=False)
    for i, h in enumerate(hist):
        assert not len(np.intersect1d(got[0][i], h))
        ok = np.ones(500, bool)
        ok[h] = False
        T.check_tolerant(got[0][i], got[1][i], int(got[2][i]), s64[i], ok, k, tol[i])
        T.check_tolerant(free[0][i], free[1][i], int(free[2][i]), s64[i], np.ones(500, bool), k, tol[i])
    assert len(np.intersect1d(np.argsort(-s64[0])[:k], hist[0])) >= 5, "the fp64 list holds no history item"
    assert len(np.intersect1d(free[0][0], hist[0])) >= 5


def test_similar_items_is_the_cosine_topk():
    from dcrecommend.nn import rank
    p, X, Y = _served()
    m = _model(p, 40.0, X, Y)
    items = np.array([0, 499, 64, 64, 250])
    got = m.similar_items(items, 15)
    for i, it in enumerate(items):
        assert it not in got[0][i]
    Yd = torch.from_numpy(Y).to(DEV)
    want = rank.TopK(*rank.identity_csr(500), None, DEV, n_cand=500).topk(Yd, Yd, items, 15)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[2], want[2])


def test_evaluate_topk_against_the_reference_metrics():
    p, X, Y = _served()
    m = _model(p, 40.0, X, Y)
    rs = np.random.RandomState(12)
    truth = [np.sort(rs.choice(500, rs.randint(0, 9), replace=False)) for _ in range(300)]
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in truth])]).astype(np.int64)
    tidx = np.concatenate(truth).astype(np.int32)
    eptr, eidx, _ = W.csr(p["rows"], p["cols"], None, 300)
    eidx = eidx.astype(np.int32)
    ks = (5, 10, 33)
    res = m.evaluate_topk(tptr, tidx, ks=ks, exclude_ptr=eptr, exclude_idx=eidx, per_user=True)
    users = np.flatnonzero(np.diff(tptr) > 0)
    assert res["users"] == users.tolist() and res["n_users"] == len(users)
    lists = m.recommend(users, max(ks), exclude_seen=True)
    exposure = np.zeros((len(ks), 500), np.int64)
    per, flags = M.metrics(lists[0], lists[2], users, tptr, tidx, list(ks), 500, exposure)
    mean, n = M.means(per, flags)
    cov = M.coverage(exposure, None, 500)
    assert n == res["n_users"]
    np.testing.assert_allclose(res["per_user"], per, rtol=0, atol=1e-12)
    for s, name in enumerate(M.NAMES):
        for i, k in enumerate(ks):
            assert abs(res["%s@%d" % (name, k)] - mean[i, s]) <= 1e-12, (name, k)
    for i, k in enumerate(ks):
        assert abs(res["coverage@%d" % k] - cov[i]) <= 1e-12
    # explicit users, one of them without truth
    empty = int(np.flatnonzero(np.diff(tptr) == 0)[0])
    sub = m.evaluate_topk(tptr, tidx, ks=ks, users=[int(users[0]), empty, int(users[5])], exclude_ptr=eptr,
                          exclude_idx=eidx)
    assert sub["n_users"] == 2 and set(sub) == {"n_users"} | {"%s@%d" % (nm, k) for nm in M.NAMES + ("coverage",)
                                                             for k in ks}


# ------------------------------------------------------------------------------------- DCBR cold start
def test_dcbr_hybrid_table_and_cold_recommendations():
    from dcrecommend.dcbr import DCBR
    torch.manual_seed(3)
    n_users, n_items, d = 30, 40, 16
    cold = np.array([2, 5, 8, 13, 21, 22, 30, 31, 38, 39])
    rs = np.random.RandomState(21)
    pick = rs.rand(n_users, n_items) < 0.3
    pick[:, cold] = False
    pick[np.arange(n_users), np.setdiff1d(np.arange(n_items), cold)[np.arange(n_users) % 30]] = True  # no empty warm item
    rows, cols = np.nonzero(pick)
    p = dict(rows=rows, cols=cols, values=None, n_users=n_users, n_items=n_items, d=d,
             X=(rs.randn(n_users, d) * 0.3).astype(np.float32), Y=(rs.randn(n_items, d) * 0.3).astype(np.float32))
    m = _model(p, 10.0)
    assert np.array_equal(np.flatnonzero(np.bincount(cols, minlength=n_items) == 0), cold)
    net = DCBR(feature_dim=d, conv_hidden=16, device=DEV)
    tracks = torch.randn(n_items, 131, 128, device=DEV).half()
    table = net.hybrid_item_factors(m, tracks)
    assert net.net.training
    pred = net.predict(tracks, torch.as_tensor(cold, device=DEV))
    warm = np.setdiff1d(np.arange(n_items), cold)
    assert torch.equal(table[cold], pred) and torch.equal(table[warm], m.item_factors[warm])
    assert table.data_ptr() != m.item_factors.data_ptr() and torch.equal(m.item_factors.cpu(), torch.from_numpy(p["Y"]))
    assert torch.equal(net.hybrid_item_factors(m, tracks, cold=cold[:3])[cold[:3]], pred[:3])
    # item_factors in chunks is predict per chunk
    allf = net.item_factors(tracks, batch=16)
    assert tuple(allf.shape) == (n_items, d) and torch.equal(allf[:16], net.predict(tracks, torch.arange(16, device=DEV)))
    users = np.arange(n_users)
    got = net.recommend(m, users, 5, tracks, cold_only=True)
    assert np.all(np.isin(got[0][got[0] >= 0], cold)) and np.all(got[2] == 5)
    full = net.recommend(m, users, 5, tracks)
    s64 = p["X"].astype(np.float64) @ table.cpu().numpy().astype(np.float64).T
    ptr, idx, _ = W.csr(rows, cols, None, n_users)
    tol = _tol(p["X"], table.cpu().numpy(), users, d)
    for u in users:
        ok = T.eligible(s64[u], int(u), ptr, idx, None)
        T.check_tolerant(full[0][u], full[1][u], int(full[2][u]), s64[u], ok, 5, tol[u])
    other = DCBR(feature_dim=32, conv_hidden=16, device=DEV)
    with pytest.raises(ValueError):
        other.hybrid_item_factors(m, tracks)
