"""Host side of the top-K recommendation path (include/dcue.h dcue_topk, ABI 17), no GPU needed: the
numpy reference of the selection against a brute-force sort, the workspace formula, every
bad-argument return (dcue_topk validates on the host before its first device call) and the compiled
kernels' scratch use."""
import ctypes
import os
import re

import numpy as np
import pytest

import topk_reference as T
from conftest import ROOT
from kernel_resources import HIPCC, kernel_resources

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


# ------------------------------------------------------------------------------- the reference
def _brute(scores_row, row, k, excl, mask):
    items = []
    for c, s in enumerate(scores_row):
        if s != s or (mask is not None and not mask[c]) or c in excl.get(row, ()):
            continue
        items.append((-s, c))
    items.sort()
    return [c for _, c in items[:k]], [-s for s, _ in items[:k]]


def _csr(excl, n_rows):
    ptr = np.zeros(n_rows + 1, np.int64)
    idx = []
    for r in range(n_rows):
        idx += sorted(excl.get(r, ()))
        ptr[r + 1] = len(idx)
    return ptr, np.array(idx, np.int32)


def test_reference_matches_brute_force():
    # row 0: ties (candidates 1, 3, 4 at 0.5) and the best item (2) excluded; row 1: fewer than K
    # eligible; row 2: a NaN score and a masked best
    scores = np.array([[0.25, 0.5, 0.9, 0.5, 0.5, -1.0, 0.0],
                       [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7],
                       [np.nan, 1.0, 0.0, 0.0, -0.5, 0.75, 0.75]])
    excl = {0: {2}, 1: {0, 1, 2, 6}}
    mask = np.array([1, 1, 1, 1, 1, 1, 1], np.uint8)
    mask2 = np.array([1, 0, 1, 1, 1, 1, 1], np.uint8)
    ptr, idx = _csr(excl, 3)
    for m in (None, mask, mask2):
        for k in (1, 3, 5, 7):
            got = T.topk(None, None, [0, 1, 2, 1], k, ptr, idx, m, scores=scores[[0, 1, 2, 1]])
            for i, row in enumerate([0, 1, 2, 1]):
                want_idx, want_s = _brute(scores[row], row, k, excl, m)
                n = len(want_idx)
                assert got[2][i] == n
                assert got[0][i, :n].tolist() == want_idx and got[1][i, :n].tolist() == want_s
                assert np.all(got[0][i, n:] == -1) and np.all(np.isneginf(got[1][i, n:]))
    got = T.topk(None, None, [0], 3, ptr, idx, None, scores=scores[[0]])
    assert got[0][0].tolist() == [1, 3, 4]  # the excluded best is gone; ties by ascending index
    got = T.topk(None, None, [1], 5, ptr, idx, None, scores=scores[[1]])
    assert got[2][0] == 3 and got[0][0].tolist() == [5, 4, 3, -1, -1]
    got = T.topk(None, None, [2], 2, None, None, mask2, scores=scores[[2]])
    assert got[0][0].tolist() == [5, 6]  # NaN never selected, the masked 1.0 neither


def test_reference_cosine_clamp():
    q = np.array([[3.0, 4.0], [0.0, 0.0]])
    c = np.array([[6.0, 8.0], [0.0, 0.0], [-3.0, -4.0]])
    s = T.cosines(q, c, [0, 1])
    np.testing.assert_allclose(s, [[1.0, 0.0, -1.0], [0.0, 0.0, 0.0]], atol=1e-15)


def test_tolerant_check_accepts_exact_and_rejects_wrong():
    rs = np.random.RandomState(0)
    s = rs.randn(200)
    ok = rs.rand(200) < 0.8
    idx, sc, n = T.select(s, ok, 10)
    T.check_tolerant(idx, sc.astype(np.float32), n, s, ok, 10, 1e-6)
    bad = idx.copy()
    bad[3] = np.flatnonzero(ok)[np.argmin(s[ok])]  # the worst eligible item in place of a top one
    with pytest.raises(AssertionError):
        T.check_tolerant(bad, sc.astype(np.float32), n, s, ok, 10, 1e-6)


# ------------------------------------------------------------------------------- workspace
def _ws(n_cand, d, qb, k, split):
    from dcrecommend import _native as nat
    n = ctypes.c_size_t(0)
    st = nat.lib().dcue_topk_workspace_bytes(n_cand, d, qb, k, split, ctypes.byref(n))
    return st, n.value


@pytest.mark.parametrize("d", [16, 100, 128, 256])
@pytest.mark.parametrize("k", [1, 100, 128])
def test_workspace_bytes(d, k):
    st, base = _ws(200000, d, 4096, k, 0)
    assert st == OK and base > 0
    dp = (d + 15) // 16 * 16
    assert base >= 200000 * dp * 4, "the normalised candidates live in the workspace"
    for split in (0, 1, 5):
        sizes = [_ws(200000, d, qb, k, split)[1] for qb in (1, 16, 64, 1000, 4096, 20000)]
        assert sizes == sorted(sizes), ("query_batch", split, sizes)
        sizes = [_ws(200000, d, 4096, kk, split)[1] for kk in sorted({1, 2, 10, 100, 128, k})]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], ("k", split, sizes)
    sizes = [_ws(200000, d, 4096, k, s)[1] for s in (1, 2, 5, 16, 32)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1], ("cand_split", sizes)
    # the partial keys: query_batch x cand_split x k x 8 bytes more than without them
    assert _ws(200000, d, 4096, k, 2)[1] - _ws(200000, d, 4096, k, 1)[1] >= 4096 * k * 8


def test_workspace_config2_bound():
    """BASELINE config 2: no [query_batch][n_cand] buffer -- under a quarter of the score matrix."""
    st, n = _ws(200000, 128, 4096, 100, 0)
    assert st == OK and n < 4096 * 200000 * 4 // 4
    from dcrecommend import _native as nat
    assert nat.TOPK_MAX_K == 128
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_TOPK_MAX_K (\d+)", hdr).group(1)) == nat.TOPK_MAX_K
    assert nat.ABI_VERSION == 17 and nat.lib().dcue_abi_version() == 17


# ------------------------------------------------------------------------------- bad arguments
def test_workspace_bytes_errors():
    from dcrecommend import _native as nat
    assert _ws(1000, 64, 64, 0, 0)[0] == INVALID
    assert _ws(1000, 64, 64, 129, 0)[0] == INVALID
    assert _ws(0, 64, 64, 10, 0)[0] == INVALID
    assert _ws(1000, 64, 0, 10, 0)[0] == INVALID
    assert _ws(1000, 64, 64, 10, -1)[0] == INVALID
    assert nat.lib().dcue_topk_workspace_bytes(1000, 64, 64, 10, 0, None) == INVALID
    assert _ws(1000, 257, 64, 10, 0)[0] == UNSUPPORTED
    assert _ws(1000, 256, 64, 128, 0)[0] == OK


def _call(**over):
    """dcue_topk with never-dereferenced host addresses: every case returns before a device call."""
    from dcrecommend import _native as nat
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(query_feat=p, n_query_rows=10, cand_feat=p, n_cand=1000, d=64, queries=p, n_queries=4, excl_ptr=p,
             excl_idx=p, cand_mask=p, k=10, query_batch=64, cand_split=0, ws=p, ws_bytes=0, out_idx=p,
             out_score=p, out_count=p, out_flags=p, stream=None)
    a.update(over)
    order = ("query_feat", "n_query_rows", "cand_feat", "n_cand", "d", "queries", "n_queries", "excl_ptr",
             "excl_idx", "cand_mask", "k", "query_batch", "cand_split", "ws", "ws_bytes", "out_idx", "out_score",
             "out_count", "out_flags", "stream")
    return nat.lib().dcue_topk(*[a[n] for n in order])


@pytest.mark.parametrize("name", ["query_feat", "cand_feat", "queries", "ws", "out_idx", "out_score", "out_count",
                                  "out_flags"])
def test_topk_null_pointer_is_invalid(name):
    assert _call(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(n_cand=0), dict(query_batch=0),
                                  dict(cand_split=-1), dict(excl_ptr=None), dict(excl_idx=None)])
def test_topk_bad_argument_is_invalid(over):
    assert _call(**over) == INVALID


def test_topk_unsupported_and_workspace():
    assert _call(d=257) == UNSUPPORTED
    # valid arguments, a workspace of 0 bytes: refused on the host
    assert _call() == WORKSPACE
    assert _call(excl_ptr=None, excl_idx=None, cand_mask=None) == WORKSPACE
    assert _call(n_queries=0) == OK  # nothing to do


# ------------------------------------------------------------------------------- compiled kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_topk_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("topk.hip", tmp_path)
    for kern in ("k_topk_scores", "k_topk_merge"):
        found = {k: v for k, v in res.items() if kern in k}
        assert found, "no %s instance found" % kern
        for k, v in found.items():
            assert v.get("ScratchSize", -1) == 0, (k, v)
