"""dcue_rank_metrics (csrc/rank.hip: five kernels and rank_sort.h's bitonic sort) against the fp64 oracle
at the list sizes and batches it serves, and dcue_factor_repeat_mean bit for bit.

Every case of tests/rank_regime_cases.py has exactly representable scores (tests/test_rank_regimes_cpu.py
proves it per case), so has_pos is held equal and auc / ap to atol = 1e-12, rtol = 0 --
test_gpu_eval.test_rank_metrics_lattice_exact's bar -- at the regimes that test's one shape leaves trivial:

  case          n (in-list positives)         candidates: 8,192-chunks   queries per pass (64-tiles)   d
  threshold     0 1 2 255 256 257 511 512     9,001: 2, last of 809      16, 3                         32
                513 1,024 4,095 4,096
  cap-*         the above + one row of 4,097  9,001: 2                   over-cap query first / 6th    32
                                                                         of pass 1, 2nd of pass 2
  cand<N>       0 .. min(300, listed)         N = 1 63 64 65 8,191       60                            16
                                              8,192: 1; 8,193: 2, last
                                              of 1; 20,001: 3, last of
                                              3,617
  pass<QB>      0 .. 150                      8,193: 2, last of 1        QB = 1 5 (C entry point) 16   100
                                                                         63 64 65 128 257 300 1,000:
                                                                         up to 5 tiles, short last
                                                                         pass
  width<D>      0 .. 150                      2,500: 1                   64, 64, 22                    1 2 3 4 7 15 16
                                                                                                       17 20 255 256
  identical-d*  0 .. 300, one run             2,500: 1                   60                            1, 16
  tie-d1        0 1 600 2,500 4,000: runs     8,000: 1                   30                            1
                of 300, 1,250, 2,000
  degenerate-*  0 .. 150 / every list item    600: 1                     16, 16, 8                     16
  nonfinite     20 .. 300                     20,001: 3, last of 3,617   128, 72 (2 tiles)             128

n <= 256 sorts with one compare-exchange per thread and scans one bin per thread; above that the sort's
and the scan's per-thread loops and k_rank_finalize's strided loop take more than one trip. Every case
runs in both modes (DCUE.score's split lists, DCUE.score_song's single list).
"""
import ctypes

import numpy as np
import pytest
import torch

import rank_regime_cases as C
from oracle import rank_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _evaluator(c):
    from dcrecommend.nn import rank
    return rank.RankEvaluator(c.inp, DEV, max_score_bytes=4 * len(c.cand) * c.qb)


def _direct(ev, qf, cand, queries, mode, qb):
    """RankEvaluator.metrics' call with query_batch as given (the binding floors it at 16): the same
    buffers, a workspace of dcue_rank_workspace_bytes, no non-finite flag expected."""
    from dcrecommend import _native as nat
    q = _dev(np.asarray(queries, np.int32))
    nq, d = int(q.numel()), int(qf.shape[1])
    auc = torch.zeros(nq, dtype=torch.float64, device=DEV)
    ap = torch.zeros_like(auc)
    flag = torch.zeros(nq, dtype=torch.int32, device=DEV)
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib().dcue_rank_workspace_bytes(ev.n_cand, d, qb, ctypes.byref(nbytes)), "dcue_rank_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    nat.check(nat.lib().dcue_rank_metrics(
        nat.ptr(qf), qf.shape[0], nat.ptr(cand), ev.n_cand, d, nat.ptr(q), nq, nat.ptr(ev.pos_ptr),
        nat.ptr(ev.pos_idx), nat.ptr(ev.cand_class), int(mode), int(qb), nat.ptr(ws), ws.numel(), nat.ptr(auc),
        nat.ptr(ap), nat.ptr(flag), nat.stream_handle(torch.device(DEV))), "dcue_rank_metrics")
    flag = flag.cpu().numpy()
    assert not (flag & 2).any()
    return auc.cpu().numpy(), ap.cpu().numpy(), (flag & 1).astype(bool)


def _metrics(c, ev=None, queries=None):
    ev = ev or _evaluator(c)
    queries = c.queries if queries is None else queries
    if c.direct:
        return _direct(ev, _dev(c.qf), _dev(c.cand), queries, c.mode, c.qb)
    return ev.metrics(_dev(c.qf), _dev(c.cand), queries, c.mode)


def _hold_to_oracle(c, got, want, queries=None):
    """has_pos equal, auc / ap within 1e-12; a miss names the case, the query, its n and where it sat."""
    queries = c.queries if queries is None else queries
    auc, ap, ok = got
    want_auc, want_ap, want_ok = want
    miss = (ok != want_ok.astype(bool)) | ~(np.abs(auc - want_auc) <= 1e-12) | ~(np.abs(ap - want_ap) <= 1e-12)
    if miss.any():
        k = int(np.argmax(miss))
        eff = c.qb if c.direct else max(16, min(len(queries), c.qb))
        print("%s (mode %d): %d of %d queries miss; first at position %d (row %d, n = %d): pass %d, query tile %d "
              "of it; %d candidate chunk(s); auc %.17g want %.17g, ap %.17g want %.17g, has_pos %d want %d"
              % (c.name, c.mode, int(miss.sum()), len(queries), k, queries[k], C.in_list_positives(c)[queries[k]],
                 k // eff, (k % eff) // C.TILE, c.facts["chunks"], auc[k], want_auc[k], ap[k], want_ap[k],
                 ok[k], want_ok[k]))
    assert np.array_equal(ok, want_ok.astype(bool))
    np.testing.assert_allclose(auc, want_auc, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ap, want_ap, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(C.CASES))
def test_rank_metrics_regime(name):
    c = C.get(name)
    _hold_to_oracle(c, _metrics(c), C.oracle(name))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("place", list(C.CAP_PLACES))
def test_rank_metrics_cap_then_valid(mode, place):
    """A query with 4,097 positives inside the lists is DCUE_ERR_UNSUPPORTED wherever it sits; the
    evaluator's next call (the status word is reset per call) is the oracle's again."""
    c = C.cap_case(mode, place)
    ev = _evaluator(c)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        _metrics(c, ev, c.facts["bad_queries"])
    _hold_to_oracle(c, _metrics(c, ev), C.oracle("threshold-m%d" % mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_metrics_batching_invariant(mode):
    """auc, ap and flags do not depend on query_batch, bit for bit, and are the oracle's."""
    first = None
    for qb in C.PASS_QBS:
        c = C.get("pass%d-m%d" % (qb, mode))
        got = _metrics(c)
        first = first or got
        for a, b in zip(got, first):
            assert np.array_equal(a, b), "query_batch %d differs from %d" % (qb, C.PASS_QBS[0])
    _hold_to_oracle(c, first, C.oracle(c.name))


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_metrics_batching_invariant_gaussian(mode):
    """The same for scores of general values (gaussian factors), GPU against GPU only: a score is one
    dot product in a fixed k order wherever its tile sits, the histograms are integer atomics, the sort
    is over full keys and the fp64 sums run in thread order. (Not held to the oracle, where scores less
    than an ulp apart may legitimately order differently.)"""
    first = None
    for qb in C.PASS_QBS:
        c = C.pass_case(mode, qb, gaussian=True)
        got = _metrics(c)
        first = first or got
        for a, b, what in zip(got, first, ("auc", "ap", "has_pos")):
            assert np.array_equal(a, b), "%s: query_batch %d differs from %d" % (what, qb, C.PASS_QBS[0])
    assert first[2].any() and np.all((first[0] >= 0) & (first[0] <= 1))


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_metrics_nonfinite_at_scale(mode):
    """NaN factors beyond the first histogram chunk and the first query tile: the evaluator raises
    where the oracle does (test_gpu_eval.test_rank_metrics_nonfinite_raise at 20,001 candidates), and
    NaN candidates of no list change no bit."""
    c = C.get("nonfinite-m%d" % mode)
    ev = _evaluator(c)
    clean = ev.metrics(_dev(c.qf), _dev(c.cand), c.queries, mode)
    for name, qf, cand, queries, raises, same, oracle_queries in C.nonfinite_variants(c):
        err = []
        for fn in (lambda: ev.metrics(_dev(qf), _dev(cand), queries, mode),
                   lambda: R.rank_metrics(qf, cand, oracle_queries, c.inp["pos_ptr"], c.inp["pos_idx"],
                                          c.inp["cand_class"], mode)):
            try:
                out = fn()
                err.append(None)
            except ValueError as e:
                err.append(str(e))
            if same and not err[-1] and len(out[0]) == len(clean[0]):
                assert np.array_equal(out[0], clean[0]) and np.array_equal(out[1], clean[1]), name
                assert np.array_equal(out[2], clean[2]), name
        assert [bool(e) for e in err] == [raises, raises], (name, err)
        assert not raises or "Input contains NaN" in err[0], (name, err)


REPEAT_N = [1, 255, 256, 257, 100 * 128 + 3]
REPEAT_ITERS = [1, 2, 3, 10]


def _repeat_values(n, seed):
    """Gaussians scaled by 1e-20, 1 and 1e20 in turn (no subnormals), then +-0.0 and a value whose
    ten-fold sum overflows, at the front of what fits."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n) * np.array([1e-20, 1.0, 1e20])[np.arange(n) % 3]).astype(np.float32)
    special = np.array([5e37, 0.0, -0.0, 1.0], np.float32)
    x[:min(n, 4)] = special[(np.arange(min(n, 4)) + seed) % 4]
    assert not np.any((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny))
    return torch.from_numpy(x)


@pytest.mark.parametrize("n_iter", REPEAT_ITERS)
@pytest.mark.parametrize("n", REPEAT_N)
def test_factor_repeat_mean_bits(n, n_iter):
    from dcrecommend import _native as nat
    for seed in range(4 if n == 1 else 1):  # n = 1: each special value in turn
        x = _repeat_values(n, seed)
        want = R.item_factors_avg(x, n_iter)
        f = x.to(DEV)
        nat.check(nat.lib().dcue_factor_repeat_mean(nat.ptr(f), n, n_iter, nat.stream_handle(torch.device(DEV))),
                  "dcue_factor_repeat_mean")
        got = f.cpu()
        assert torch.equal(got, want), (n, n_iter, seed)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, n_iter, seed)  # the sign of zero too
    if n_iter == 10 and n >= 4:
        assert torch.isinf(want).sum() == 1


def test_factor_repeat_mean_edges():
    from dcrecommend import _native as nat
    x = _repeat_values(257, 0)
    f = x.to(DEV)
    s = nat.stream_handle(torch.device(DEV))
    assert nat.lib().dcue_factor_repeat_mean(nat.ptr(f), 0, 10, s) == 0  # DCUE_OK, nothing touched
    assert nat.lib().dcue_factor_repeat_mean(nat.ptr(f), 257, 0, s) == 1  # DCUE_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(f.cpu().view(torch.int32), x.view(torch.int32))
