"""Host side of the WRMF serving path (include/dcue.h dcue_topk_scored, dcue_wrmf_objective; ABI 17),
no GPU needed: the sparse identity's numpy restatement against the dense fp64 oracle, every
bad-argument return (both calls validate on the host before their first device call), the workspace
formula and the compiled kernels' scratch use."""
import ctypes
import functools
import os

import numpy as np
import pytest

import wrmf_serve_reference as R
from kernel_resources import HIPCC, kernel_resources
from oracle import wrmf_oracle as W

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
ALPHA, LAM = 40.0, 0.05
SHAPES = {"300x500": (300, 500, 100, True), "257x131": (257, 131, 128, False), "40x33": (40, 33, 7, True)}


# ------------------------------------------------------------------------------- the identity
@functools.lru_cache(maxsize=None)
def _problem(name):
    nu, ni, d, vals = SHAPES[name]
    return R.problem(11 + nu, nu, ni, d, vals)


@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sparse_identity_matches_dense_oracle(name, iters):
    """Measured with numpy on the CPU: a relative difference of at most 2.6e-14 over these cases."""
    p = _problem(name)
    X, Y = (p["X"], p["Y"]) if iters == 0 else R.als_iterations(p, ALPHA, LAM, iters)
    want = W.objective(X, Y, p["rows"], p["cols"], p["values"], ALPHA, LAM)
    got = R.objective_terms(X, Y, p["rows"], p["cols"], p["values"], ALPHA, LAM)
    print("%s iters=%d: dense %.17g sparse %.17g rel %.3e" % (name, iters, want, got[0], abs(got[0] - want) / abs(want)))
    assert abs(got[0] - want) <= 1e-12 * abs(want)
    assert got[0] == got[1] + got[2] + got[3]


# ------------------------------------------------------------------------------- dcue_topk_scored
def _scored(score, **over):
    """dcue_topk_scored with never-dereferenced host addresses: every case returns before a device call."""
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
    return nat.lib().dcue_topk_scored(score, *[a[n] for n in order])


@pytest.mark.parametrize("score", [2, -1])
def test_scored_unknown_score_is_invalid(score):
    assert _scored(score) == INVALID
    assert _scored(score, n_queries=0) == INVALID  # before "nothing to do", too


@pytest.mark.parametrize("score", [0, 1])
@pytest.mark.parametrize("name", ["query_feat", "cand_feat", "queries", "ws", "out_idx", "out_score", "out_count",
                                  "out_flags"])
def test_scored_null_pointer_is_invalid(score, name):
    assert _scored(score, **{name: None}) == INVALID


@pytest.mark.parametrize("score", [0, 1])
@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(n_cand=0), dict(query_batch=0), dict(cand_split=-1),
                                  dict(excl_ptr=None), dict(excl_idx=None), dict(n_query_rows=0), dict(n_queries=-1),
                                  dict(d=0)])
def test_scored_bad_argument_is_invalid(score, over):
    assert _scored(score, **over) == INVALID


@pytest.mark.parametrize("score", [0, 1])
def test_scored_unsupported_and_workspace(score):
    assert _scored(score, d=257) == UNSUPPORTED
    assert _scored(score) == WORKSPACE  # valid arguments, a workspace of 0 bytes: refused on the host
    assert _scored(score, excl_ptr=None, excl_idx=None, cand_mask=None) == WORKSPACE
    assert _scored(score, n_queries=0) == OK  # nothing to do


def test_score_constants_match_the_header():
    import re

    from conftest import ROOT
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_SCORE_COSINE (\d+)", hdr).group(1)) == nat.SCORE_COSINE == 0
    assert int(re.search(r"#define DCUE_SCORE_DOT (\d+)", hdr).group(1)) == nat.SCORE_DOT == 1
    assert nat.ABI_VERSION == 17 and nat.lib().dcue_abi_version() == 17


# ------------------------------------------------------------------------------- dcue_wrmf_objective
def _obj_ws(n_users, n_items, dim):
    from dcrecommend import _native as nat
    n = ctypes.c_size_t(0)
    st = nat.lib().dcue_wrmf_objective_workspace_bytes(n_users, n_items, dim, ctypes.byref(n))
    return st, n.value


def _objective(**over):
    from dcrecommend import _native as nat
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(X=p, n_users=100, Y=p, n_items=200, dim=64, indptr=p, indices=p, values=p, alpha=40.0, lam=0.1, ws=p,
             ws_bytes=1 << 40, out=p, stream=None)
    a.update(over)
    order = ("X", "n_users", "Y", "n_items", "dim", "indptr", "indices", "values", "alpha", "lam", "ws", "ws_bytes",
             "out", "stream")
    return nat.lib().dcue_wrmf_objective(*[a[n] for n in order])


@pytest.mark.parametrize("name", ["X", "Y", "indptr", "indices", "ws", "out"])
def test_objective_null_pointer_is_invalid(name):
    assert _objective(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(dim=0), dict(dim=-3), dict(dim=129), dict(lam=0.0), dict(lam=-1.0),
                                  dict(lam=float("nan")), dict(n_users=-1), dict(n_items=-1)])
def test_objective_bad_argument_is_invalid(over):
    assert _objective(**over) == INVALID


def test_objective_workspace_too_small():
    st, need = _obj_ws(100, 200, 64)
    assert st == OK and need > 0
    assert _objective(ws_bytes=need - 1) == WORKSPACE
    assert _objective(ws_bytes=0) == WORKSPACE


def test_objective_workspace_bytes_errors():
    from dcrecommend import _native as nat
    assert nat.lib().dcue_wrmf_objective_workspace_bytes(100, 200, 64, None) == INVALID
    for bad in [(100, 200, 0), (100, 200, 129), (-1, 200, 64), (100, -1, 64)]:
        assert _obj_ws(*bad)[0] == INVALID
    assert _obj_ws(0, 0, 1)[0] == OK and _obj_ws(100, 200, 128)[0] == OK


def test_objective_workspace_is_monotone():
    for dim in (1, 7, 100, 128):
        sizes = [_obj_ws(100000, ni, dim)[1] for ni in (0, 1, 511, 512, 513, 200000, 262144, 262145, 10 ** 7)]
        assert sizes == sorted(sizes), ("n_items", dim, sizes)
        sizes = [_obj_ws(nu, 200000, dim)[1] for nu in (0, 1, 4096, 4097, 100000, 10 ** 7, 2 * 10 ** 7)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], ("n_users", dim, sizes)
    for nu, ni in ((100000, 200000), (300, 500), (1, 1)):
        sizes = [_obj_ws(nu, ni, dim)[1] for dim in (1, 7, 16, 17, 100, 127, 128)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], ("dim", nu, ni, sizes)
    # config 2 (100k x 200k, d = 128): the Gram partials and one double per user, nowhere near the
    # 160 GB of the dense fp64 matrix
    assert _obj_ws(100000, 200000, 128)[1] < 64 << 20


# ------------------------------------------------------------------------------- compiled kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_objective_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("wrmf_objective.hip", tmp_path)
    for kern in ("k_wrmf_obj_pairs", "k_wrmf_obj_reduce", "k_wrmf_obj_final"):
        assert any(kern in k for k in res), "no %s instance found" % kern
    assert sum("k_wrmf_obj_pairs" in k for k in res) == 2  # the 16-byte and the 4-byte row loads
    for k, v in res.items():
        assert v.get("ScratchSize", -1) == 0, (k, v)
