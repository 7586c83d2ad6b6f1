"""The cases of tests/rank_regime_cases.py keep their promises (no GPU): from the inputs alone, the
in-list positive counts, the 8,192-candidate chunks, the passes and their query tiles and the runs of
equal thresholds are what each case says, and the oracle's numbers (torch's fp32 CPU cosine) equal an
integer restatement of the scores bit for bit -- so the 1e-12 the GPU test holds is a condition the
inputs meet. A seed or a class mix that drifts fails here before a GPU case silently stops reaching its
regime. Each test prints the case's regime facts and the oracle's time.
"""
import time

import numpy as np
import pytest

import rank_regime_cases as C
from oracle import rank_oracle as R


def _has_pred(c):
    ptr, idx, cls = c.inp["pos_ptr"], c.inp["pos_idx"], c.inp["cand_class"]
    return np.array([bool((cls[idx[ptr[r]:ptr[r + 1]]] & 1).any()) for r in range(len(ptr) - 1)])


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_keeps_its_promises(name, capsys):
    c = C.get(name)
    f = c.facts
    n_cand, d = c.cand.shape
    assert c.qf.shape == (len(c.inp["pos_ptr"]) - 1, d) and len(c.inp["cand_class"]) == n_cand
    assert d == f["d"] and c.queries.min() >= 0 and c.queries.max() < len(c.qf)
    # positives inside the lists, per row, and over the rows that are asked
    n = C.in_list_positives(c)
    assert np.array_equal(n, f["row_n"])
    asked = n[c.queries]
    assert asked.max() <= C.CAP
    if "n_set" in f:
        assert set(asked.tolist()) == f["n_set"]
        assert len(set(c.queries.tolist())) < len(c.queries), "some rows are asked twice"
        ptr = c.inp["pos_ptr"]
        assert any(ptr[q + 1] - ptr[q] > C.CAP and n[q] == C.CAP for q in c.queries)
        assert n[13] == C.CAP + 1 and 13 not in c.queries
    if "n_max" in f:
        assert asked.min() == 0 and asked.max() == f["n_max"]
    # candidate chunks of k_rank_hist, passes and query tiles of k_rank_scores
    chunks = -(-n_cand // C.CHUNK)
    assert (f["chunks"], f["last_chunk"]) == (chunks, n_cand - (chunks - 1) * C.CHUNK)
    if chunks > 1:  # the candidates at the chunks' edges are in both lists: no mode leaves them out
        assert (c.inp["cand_class"][[C.CHUNK - 1, C.CHUNK, -1]] == 3).all()
    eff = c.qb if c.direct else max(16, min(len(c.queries), c.qb))  # the binding's floor and cap
    assert f["passes"] == C.passes(len(c.queries), eff) and sum(f["passes"]) == len(c.queries)
    # runs of equal thresholds
    runs = {row: C.longest_threshold_run(c, row) for row in f["runs"]}
    for row, least in f["runs"].items():
        assert row in c.queries and runs[row] >= least, (row, runs[row], least)
    # the oracle, and its scores restated in integers
    t0 = time.perf_counter()
    want = C.oracle_of(c)
    took = time.perf_counter() - t0
    with capsys.disabled():  # the facts and the time belong in the run's output, passing or not
        print("\n%s: n in [%d, %d], %d chunk(s), last of %d, passes %s (%d tile(s) at most), d = %d, runs %s; "
              "oracle %.2f s" % (name, asked.min(), asked.max(), chunks, f["last_chunk"],
                                 f["passes"] if len(f["passes"]) <= 6 else "%d x %d" % (len(f["passes"]), f["passes"][0]),
                                 -(-max(f["passes"]) // C.TILE), d, runs, took))
    assert took < 5.0
    got = C.restated_metrics(c)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    if f.get("all_tie") and c.mode == 1:
        both = (asked > 0) & bool((c.inp["cand_class"] & 1).any())
        assert both.any() and np.all(want[0][both] == 0.5)


def test_regimes_are_reached():
    """What the issue's table asks for exists among the cases: the shape facts, not their values."""
    get = C.get
    for mode in (0, 1):
        t = get("threshold-m%d" % mode)
        assert t.facts["chunks"] == 2 and t.facts["last_chunk"] == 9001 - 8192 and len(t.facts["passes"]) == 2
        assert [get("cand%d-m%d" % (k, mode)).facts["chunks"] for k in C.CAND_COUNTS] == [1, 1, 1, 1, 1, 1, 2, 3]
        sizes = {qb: get("pass%d-m%d" % (qb, mode)).facts["passes"] for qb in C.PASS_QBS}
        assert sizes[1] == [1] * 300 and sizes[5] == [5] * 60 and sizes[16][-1] == 12
        assert sizes[63][-1] == 48 and sizes[65] == [65] * 4 + [40] and sizes[257] == [257, 43]
        assert sizes[300] == sizes[1000] == [300]  # five query tiles in one pass
        for qb in C.PASS_QBS:
            assert get("pass%d-m%d" % (qb, mode)).cand is get("pass1-m%d" % mode).cand
            assert get("pass%d-m%d" % (qb, mode)).direct == (qb < 16)
        g = C.pass_case(mode, 64, gaussian=True)
        assert g.cand.shape == (8193, 100) and np.array_equal(g.queries, get("pass64-m%d" % mode).queries)
        assert len(np.unique(g.cand @ g.qf[0])) > 4000  # general values, not a lattice
        assert max(get("nonfinite-m%d" % mode).facts["passes"]) > C.TILE


@pytest.mark.parametrize("mode", [0, 1])
def test_cap_cases(mode):
    for place, at in C.CAP_PLACES.items():
        c = C.cap_case(mode, place)
        bad = c.facts["bad_queries"]
        n = C.in_list_positives(c)[bad]
        assert n[at] == C.CAP + 1 and (np.delete(n, at) <= C.CAP).all()
        assert at // c.qb == (1 if place == "second" else 0) and (at % c.qb == 0) == (place == "first")
        assert np.array_equal(np.delete(bad, at), np.delete(c.queries, at))


@pytest.mark.parametrize("mode", [0, 1])
def test_degenerate_cases(mode):
    cls = C.get("degenerate-nobit0-m%d" % mode).inp["cand_class"]
    assert not (cls & 1).any() and (cls & 2).any()
    auc, ap, ok = C.oracle("degenerate-nobit0-m%d" % mode)
    if mode == 0:
        assert not ok.any()
    else:  # n0 = 0: every target is 1 (nn/dcue.py:466-468)
        assert np.all(auc == 1.0) and np.all(ap == 1.0)
    cls = C.get("degenerate-nobit1-m%d" % mode).inp["cand_class"]
    assert not (cls & 2).any() and (cls & 1).any()
    c = C.get("degenerate-allpos-m%d" % mode)
    cls, ptr, idx = c.inp["cand_class"], c.inp["pos_ptr"], c.inp["pos_idx"]
    assert np.array_equal(idx[ptr[0]:ptr[1]], np.flatnonzero(cls != 0))
    at = np.flatnonzero(c.queries == c.facts["other_list_row"])
    assert len(at) and 0 < at[0] < len(c.queries) - 5
    auc, ap, ok = C.oracle(c.name)
    assert not ok[at[0]] and ok[at[0] + 1] and ok[at[0] + 2:].any() and ok[:at[0]].any()
    if mode == 0:
        assert np.all(np.abs(auc[c.queries == 0] - 1.0) < 1e-15)  # both sets hold only 1s


@pytest.mark.parametrize("mode", [0, 1])
def test_nonfinite_variants(mode):
    """The oracle's verdict on each variant, and where the NaNs sit."""
    c = C.get("nonfinite-m%d" % mode)
    cls = c.inp["cand_class"]
    assert _has_pred(c)[c.queries].all() and not _has_pred(c)[c.facts["no_pred_row"]]
    assert np.flatnonzero(c.queries == c.facts["nan_row"]).tolist() == [C.NONFINITE_NAN_AT]
    assert C.TILE <= C.NONFINITE_NAN_AT % c.qb
    variants = C.nonfinite_variants(c)
    assert len(variants) == (4 if mode == 0 else 3)
    for name, qf, cand, queries, raises, same, oracle_queries in variants:
        nan_c = np.flatnonzero(np.isnan(cand).any(axis=1))
        nan_q = np.flatnonzero(np.isnan(qf).any(axis=1))
        if name == "listed-candidate":
            assert len(nan_c) == 1 and nan_c[0] >= C.CHUNK and cls[nan_c[0]] & 1
        if name == "unlisted-candidates":
            assert (cls[nan_c] == 0).all() and nan_c.min() >= C.CHUNK and (nan_c >= 2 * C.CHUNK).sum() >= 2
        if name.startswith("query"):
            assert nan_q.tolist() == [c.facts["nan_row"]] and not len(nan_c)
        if name == "query-after-break":
            assert np.flatnonzero(queries == c.facts["no_pred_row"]).tolist() == [10]
        try:
            R.rank_metrics(qf, cand, oracle_queries, c.inp["pos_ptr"], c.inp["pos_idx"], cls, mode)
            err = None
        except ValueError as e:
            err = str(e)
        assert bool(err) == raises, (name, err)
        assert not err or "Input contains NaN" in err
