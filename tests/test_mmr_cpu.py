"""Host side of diversity-aware serving (include/dcue.h dcue_list_mmr / dcue_list_ild / dcue_list_ild_mean,
added under ABI 17), no GPU needed: the numpy reference against a brute-force restatement and hand
cases, the constants and symbols of header, binding and library, every bad-argument return (all calls
validate on the host before their first device call), the Python argument checks, the compiled kernels'
scratch use and LDS sizes, and the step cap of the tolerant GPU check on the reference's own fp32
emulation."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mmr_reference as R
from conftest import ROOT
from kernel_resources import HIPCC, PKG, kernel_resources

OK, INVALID, UNSUPPORTED = 0, 1, 2


# ------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rel_mode", [R.REL_RAW, R.REL_MINMAX])
def test_reference_matches_brute_force(seed, rel_mode):
    rs = np.random.RandomState(seed)
    n_cand, d, P = 40, 5, 9
    feat = rs.randn(n_cand, d).astype(np.float32)
    lst = rs.choice(n_cand, P, replace=False)
    rel = np.sort(rs.randn(P).astype(np.float32))[::-1].copy()
    for lam in (0.0, 0.3, 0.7, 1.0):
        for c, k_out in ((P, P), (P, 4), (5, 7), (1, 3)):
            idx, score, count, flags = R.mmr(lst, rel, c, feat, k_out, lam, rel_mode)
            pos = R.mmr_brute(lst, rel, c, feat, k_out, lam, rel_mode)
            assert flags == 0 and count == len(pos) == min(k_out, c)
            assert idx[:count].tolist() == lst[pos].tolist() and np.array_equal(score[:count], rel[pos])
            assert np.all(idx[count:] == -1) and np.all(score[count:] == -np.inf)


def test_reference_lambda_one_is_the_identity():
    rs = np.random.RandomState(1)
    feat = rs.randn(30, 7).astype(np.float32)
    lst = rs.permutation(30)[:12]
    rel = np.array([3, 3, 2.5, 2.5, 2.5, 1, 1, 0, -1, -1, -2, -2], np.float32)  # ties keep the pool's order
    for rel_mode in (R.REL_RAW, R.REL_MINMAX):
        idx, score, count, _ = R.mmr(lst, rel, 12, feat, 8, 1.0, rel_mode)
        assert count == 8 and idx.tolist() == lst[:8].tolist() and np.array_equal(score, rel[:8])


def test_reference_ties_go_to_the_lowest_position():
    # four copies of two orthogonal rows, equal relevance: every f ties until a copy's twin is picked
    feat = np.array([[1, 0], [0, 1]], np.float32)
    lst = np.array([1, 0, 1, 0])
    rel = np.ones(4, np.float32)
    idx, _, count, _ = R.mmr(lst, rel, 4, feat, 4, 0.5, R.REL_RAW)
    # step 0: all tie -> position 0 (row 1); then the row-0 copies (redundancy 0) beat the twin (1):
    # position 1; then positions 2 and 3 tie at redundancy 1 -> position 2
    assert count == 4 and idx.tolist() == [1, 0, 1, 0]
    assert R.mmr_brute(lst, rel, 4, feat, 4, 0.5, R.REL_RAW) == [0, 1, 2, 3]
    lst = np.array([1, 1, 0, 0])
    assert R.mmr_brute(lst, rel, 4, feat, 4, 0.5, R.REL_RAW) == [0, 2, 1, 3]
    assert R.mmr(lst, rel, 4, feat, 4, 0.5, R.REL_RAW)[0].tolist() == [1, 0, 1, 0]


def test_reference_lambda_zero_starts_at_position_zero():
    rs = np.random.RandomState(2)
    feat = rs.randn(20, 4).astype(np.float32)
    lst = rs.permutation(20)[:6]
    rel = -np.arange(6, dtype=np.float32) - 1  # negative: lam * r' is -0
    assert R.mmr(lst, rel, 6, feat, 3, 0.0, R.REL_RAW)[0][0] == lst[0]


def test_reference_minmax_edge_cases():
    assert R.scale_rel([2, 2, 2], R.REL_MINMAX).tolist() == [0, 0, 0]  # max == min
    assert R.scale_rel([5], R.REL_MINMAX).tolist() == [0]
    assert R.scale_rel([4, 3, 2], R.REL_MINMAX).tolist() == [1, 0.5, 0]
    assert R.scale_rel([4, 3, 2], R.REL_RAW).tolist() == [4, 3, 2]
    feat = np.eye(3, dtype=np.float32)
    # all relevances equal under min-max: r' = 0, so the order is by redundancy alone, ties by position
    idx, score, _, _ = R.mmr([2, 0, 1], np.full(3, 7, np.float32), 3, feat, 3, 0.7, R.REL_MINMAX)
    assert idx.tolist() == [2, 0, 1] and score.tolist() == [7, 7, 7]


def test_reference_sims_zero_row_and_duplicates():
    feat = np.array([[3, 4], [0, 0], [-6, -8]], np.float32)
    S = R.sims(feat, [0, 1, 2, 0])
    assert np.allclose(S[0], [1, 0, -1, 1], atol=1e-15) and np.all(S[1] == 0)
    S32 = R.sims(feat, [0, 1, 2, 0], np.float32)
    assert S32.dtype == np.float32 and np.abs(S32 - S).max() <= R.tol_sim(2) and np.array_equal(S32, S32.T)


def test_reference_flags_and_short_lists():
    feat = np.eye(4, dtype=np.float32)
    rel = np.array([3, 2, 1, 0], np.float32)
    idx, score, count, flags = R.mmr([0, 9, 1, 2], rel, 4, feat, 2, 0.5, R.REL_RAW)
    assert flags == R.FLAG_BAD_INDEX and count == 0 and np.all(idx == -1) and np.all(score == -np.inf)
    assert R.mmr([0, 9, 1, 2], rel, 1, feat, 2, 0.5, R.REL_RAW)[2:] == (1, 0)  # past count: never read
    assert R.mmr([0, 1], np.array([np.nan, 1], np.float32), 2, feat, 2, 0.5, R.REL_RAW)[3] == R.FLAG_NONFINITE
    bad = feat.copy()
    bad[1, 2] = np.inf
    assert R.mmr([0, 1], rel, 2, bad, 2, 0.5, R.REL_RAW)[3] == R.FLAG_NONFINITE
    assert R.mmr([0, 1], rel, 0, feat, 2, 0.5, R.REL_RAW)[2:] == (0, 0)


def test_reference_ild():
    feat = np.array([[1, 0], [0, 1], [1, 1], [1, 0]], np.float32)
    v, flags = R.ild([0, 1, 2, 3], 4, feat, [1, 2, 3, 4])
    s = 1 / np.sqrt(2)
    want = [0.0, 1.0, (1 + (1 - s) + (1 - s)) / 3, (1 + (1 - s) + 0 + (1 - s) + 1 + (1 - s)) / 6]
    assert flags == R.FLAG_NO_PAIR and np.abs(v - want).max() <= 1e-15
    v, flags = R.ild([0, 1, 2, 3], 3, feat, [2, 4])  # n_K = min(K, c)
    assert flags == 0 and np.abs(v - [1.0, want[2]]).max() <= 1e-15
    assert R.ild([0, 1], 1, feat, [2])[1] == R.FLAG_NO_PAIR
    assert R.ild([0, 7], 2, feat, [2])[1] == R.FLAG_BAD_INDEX
    mean, n = R.ild_means([[1.0, 2.0], [9.0, 9.0], [3.0, 4.0]], [0, 1, 0])
    assert n == 2 and mean.tolist() == [2.0, 3.0]
    assert R.ild_means([[1.0]], [2])[1] == 0


def gaussian_case(d, P, rel_mode, seed, n_lists=64, n_cand=2000):
    """Lists as a top-P call leaves them: distinct candidates, relevance (cosine for raw, inner product
    for min-max) descending."""
    rs = np.random.RandomState(seed)
    feat = rs.randn(n_cand, d).astype(np.float32)
    q = rs.randn(n_lists, d).astype(np.float32)
    lists, rels = [], []
    for u in range(n_lists):
        s = feat.astype(np.float64) @ q[u].astype(np.float64)
        if rel_mode == R.REL_RAW:
            norms = np.maximum(np.linalg.norm(feat.astype(np.float64), axis=1), 1e-8)
            s = s / norms / np.linalg.norm(q[u].astype(np.float64))
        order = np.argsort(-s, kind="stable")[:P]
        lists.append(order.astype(np.int32))
        rels.append(s[order].astype(np.float32))
    return feat, np.stack(lists), np.stack(rels)


@pytest.mark.parametrize("d", [16, 100, 128, 256])
@pytest.mark.parametrize("rel_mode", [R.REL_RAW, R.REL_MINMAX])
def test_fp32_emulation_stays_inside_the_cap(d, rel_mode):
    """The GPU tests' cap (at most 1 % of a case's steps differ from the fp64 strict argmax) on the
    reference's own fp32 emulation: the tolerance passes at every step and the cap has room."""
    P, n_lists = 128, 16
    feat, lists, rels = gaussian_case(d, P, rel_mode, seed=d, n_lists=n_lists)
    for lam in (0.3, 0.7):
        steps = differ = 0
        for u in range(n_lists):
            idx, score, count, flags = R.mmr(lists[u], rels[u], P, feat, P, lam, rel_mode, dtype=np.float32)
            assert flags == 0
            s, df = R.check_greedy_tolerant(idx, score, count, lists[u], rels[u], P, feat, P, lam, rel_mode)
            steps, differ = steps + s, differ + df
        assert steps == n_lists * P and differ <= 0.01 * steps, (differ, steps)


def test_tolerant_check_rejects_a_wrong_pick():
    feat, lists, rels = gaussian_case(16, 32, R.REL_RAW, seed=3, n_lists=1)
    idx, score, count, _ = R.mmr(lists[0], rels[0], 32, feat, 32, 0.5, R.REL_RAW)
    R.check_greedy_tolerant(idx, score, count, lists[0], rels[0], 32, feat, 32, 0.5, R.REL_RAW)
    idx[[3, 20]], score[[3, 20]] = idx[[20, 3]], score[[20, 3]]
    with pytest.raises(AssertionError, match="step 3"):
        R.check_greedy_tolerant(idx, score, count, lists[0], rels[0], 32, feat, 32, 0.5, R.REL_RAW)


def test_tolerances():
    assert R.tol_sim(16) == 48 * 2.0 ** -24 and R.tol_sim(100) == R.tol_sim(112) == 240 * 2.0 ** -24
    assert R.tol_sim(256) == 528 * 2.0 ** -24 and R.tol_rel(R.REL_RAW) == 0 and R.tol_rel(R.REL_MINMAX) == 2.0 ** -22


# ------------------------------------------------------------------------------- the surface
def test_header_binding_and_library_agree():
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1))

    assert define("DCUE_MMR_REL_RAW") == nat.MMR_REL_RAW == R.REL_RAW == 0
    assert define("DCUE_MMR_REL_MINMAX") == nat.MMR_REL_MINMAX == R.REL_MINMAX == 1
    assert nat.MMR_RELS == {"raw": 0, "minmax": 1}
    assert define("DCUE_LIST_FLAG_NO_PAIR") == nat.LIST_FLAG_NO_PAIR == R.FLAG_NO_PAIR == 1
    assert define("DCUE_LIST_FLAG_BAD_INDEX") == nat.LIST_FLAG_BAD_INDEX == R.FLAG_BAD_INDEX == 2
    assert define("DCUE_LIST_FLAG_NONFINITE") == nat.LIST_FLAG_NONFINITE == R.FLAG_NONFINITE == 4
    for sym in ("dcue_list_mmr_workspace_bytes", "dcue_list_mmr", "dcue_list_ild", "dcue_list_ild_mean"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in nat._SIGS
        assert getattr(nat.lib(), sym).argtypes == nat._SIGS[sym][0]
    assert define("DCUE_ABI_VERSION") == 17
    assert nat.ABI_VERSION == 17 and nat.lib().dcue_abi_version() == 17


# ------------------------------------------------------------------------------- bad arguments
def _p():
    """A never-dereferenced non-null address: every case returns before a device call."""
    return ctypes.c_void_p(0x1000)


def _mmr(**over):
    from dcrecommend import _native as nat
    a = dict(idx=_p(), score=_p(), count=_p(), n_lists=0, pool=64, cand_feat=_p(), n_cand=1000, d=100, lam=0.5,
             rel_mode=0, k_out=10, ws=None, ws_bytes=0, out_idx=_p(), out_score=_p(), out_count=_p(), out_flags=_p(),
             stream=None)
    a.update(over)
    order = ("idx", "score", "count", "n_lists", "pool", "cand_feat", "n_cand", "d", "lam", "rel_mode", "k_out", "ws",
             "ws_bytes", "out_idx", "out_score", "out_count", "out_flags", "stream")
    return nat.lib().dcue_list_mmr(*[a[n] for n in order])


def _ild(cutoffs=(1, 5, 10), **over):
    from dcrecommend import _native as nat
    cut = (ctypes.c_int32 * max(len(cutoffs), 1))(*cutoffs)
    a = dict(idx=_p(), count=_p(), n_lists=0, k=10, cand_feat=_p(), n_cand=1000, d=100,
             cutoffs_host=ctypes.cast(cut, ctypes.c_void_p), n_cutoffs=len(cutoffs), ws=None, ws_bytes=0, out_ild=_p(),
             out_flags=_p(), stream=None)
    a.update(over)
    order = ("idx", "count", "n_lists", "k", "cand_feat", "n_cand", "d", "cutoffs_host", "n_cutoffs", "ws", "ws_bytes",
             "out_ild", "out_flags", "stream")
    return nat.lib().dcue_list_ild(*[a[n] for n in order])


def _mean(**over):
    from dcrecommend import _native as nat
    a = dict(ild=_p(), flags=_p(), n_lists=4, n_cutoffs=3, out_mean=_p(), out_n_evaluated=_p(), stream=None)
    a.update(over)
    order = ("ild", "flags", "n_lists", "n_cutoffs", "out_mean", "out_n_evaluated", "stream")
    return nat.lib().dcue_list_ild_mean(*[a[n] for n in order])


def test_nothing_to_do_is_ok():
    """(the defaults of _mmr / _ild: valid arguments, no list)"""
    assert _mmr() == OK and _mmr(pool=128, k_out=128, d=256, lam=1.0, rel_mode=1) == OK
    assert _mmr(pool=1, k_out=1, d=1, lam=0.0) == OK
    assert _ild() == OK and _ild(k=128, cutoffs=(1, 2, 3, 4, 5, 6, 7, 128), d=256) == OK


@pytest.mark.parametrize("name", ["idx", "score", "count", "cand_feat", "out_idx", "out_score", "out_count",
                                  "out_flags"])
def test_mmr_null_pointer_is_invalid(name):
    assert _mmr(**{name: None}) == INVALID
    assert _mmr(n_lists=3, **{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(pool=0), dict(pool=129), dict(k_out=0), dict(k_out=65), dict(lam=-0.01),
                                  dict(lam=1.01), dict(lam=float("nan")), dict(rel_mode=2), dict(rel_mode=-1),
                                  dict(n_cand=0), dict(n_cand=-3), dict(n_lists=-1), dict(d=0)])
def test_mmr_bad_argument_is_invalid(over):
    assert _mmr(**over) == INVALID
    assert _mmr(**dict(dict(n_lists=3), **over)) == INVALID


@pytest.mark.parametrize("over", [dict(d=257), dict(n_cand=2 ** 31 - 64)])
def test_unsupported_sizes(over):
    assert _mmr(**over) == UNSUPPORTED and _mmr(n_lists=3, **over) == UNSUPPORTED
    assert _ild(**over) == UNSUPPORTED and _ild(n_lists=3, **over) == UNSUPPORTED
    assert _mmr(n_cand=2 ** 31 - 65) == OK


@pytest.mark.parametrize("name", ["idx", "count", "cand_feat", "cutoffs_host", "out_ild", "out_flags"])
def test_ild_null_pointer_is_invalid(name):
    assert _ild(**{name: None}) == INVALID
    assert _ild(n_lists=3, **{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(n_cutoffs=0), dict(n_cutoffs=9), dict(n_cand=0),
                                  dict(n_lists=-1), dict(d=0)])
def test_ild_bad_argument_is_invalid(over):
    assert _ild(**over) == INVALID
    assert _ild(**dict(dict(n_lists=3), **over)) == INVALID


@pytest.mark.parametrize("cutoffs", [(0, 5), (-1,), (5, 5), (5, 3), (1, 5, 11), (11,), (1, 2, 3, 3)])
def test_ild_bad_cutoffs_are_invalid(cutoffs):
    assert _ild(cutoffs=cutoffs) == INVALID
    assert _ild(cutoffs=cutoffs, n_lists=3) == INVALID


@pytest.mark.parametrize("name", ["ild", "flags", "out_mean", "out_n_evaluated"])
def test_mean_null_pointer_is_invalid(name):
    assert _mean(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(n_cutoffs=0), dict(n_cutoffs=9), dict(n_lists=-1)])
def test_mean_bad_argument_is_invalid(over):
    assert _mean(**over) == INVALID


def test_workspace_bytes_is_a_host_computation():
    from dcrecommend import _native as nat
    fn = nat.lib().dcue_list_mmr_workspace_bytes
    n = ctypes.c_size_t(12345)
    assert fn(128, 256, 4096, ctypes.byref(n)) == OK and n.value == 0  # everything lives in LDS
    assert fn(1, 1, 0, ctypes.byref(n)) == OK and n.value == 0
    assert fn(128, 256, 4096, None) == INVALID
    for pool, d, nl in ((0, 16, 1), (129, 16, 1), (16, 0, 1), (16, 16, -1)):
        assert fn(pool, d, nl, ctypes.byref(n)) == INVALID
    assert fn(16, 257, 1, ctypes.byref(n)) == UNSUPPORTED


# ------------------------------------------------------------------------------- Python arguments
def test_pool_checks_name_the_limits():
    from dcrecommend.nn import rank
    assert rank.check_pool(10, None) == (10, 40) and rank.check_pool(100, None) == (100, 128)
    assert rank.check_pool(10, 10) == (10, 10) and rank.check_pool(128, None) == (128, 128)
    with pytest.raises(ValueError, match=r"1\.\.128"):
        rank.check_pool(0, None)
    with pytest.raises(ValueError, match=r"k\.\.128"):
        rank.check_pool(10, 9)
    with pytest.raises(ValueError, match=r"k\.\.128"):
        rank.check_pool(10, 129)


def test_diversify_argument_checks():
    import torch
    from dcrecommend.nn import rank
    div = rank.Diversify("cpu")
    idx, count = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    score, feat = torch.zeros((2, 4)), torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path exists
        div.mmr_raw(idx, score, count, feat, 2, 0.5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        div.ild_raw(idx, count, feat, (1, 2))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        div.ild_mean_raw(torch.zeros((2, 2), dtype=torch.float64), torch.zeros(2, dtype=torch.int32))
    for ks, match in (((), "at least 1"), ((0,), r"1\.\.128"), ((129,), r"1\.\.128"), (range(1, 10), "at most 8")):
        with pytest.raises(ValueError, match=match):
            div.ild_raw(idx, count, feat, ks)
    tk = rank.TopK(None, None, None, "cpu", n_cand=6)
    with pytest.raises(ValueError, match="diversity"):
        tk.topk_raw(torch.zeros(2, 3), feat, [0], 2, pool=4)
    with pytest.raises(ValueError, match=r"k\.\.128"):
        tk.topk_raw(torch.zeros(2, 3), feat, [0], 4, diversity=0.5, pool=2)
    ev = rank.TopKMetrics(np.array([0, 1, 2]), np.array([1, 4]), "cpu", n_cand=6)
    with pytest.raises(ValueError, match=r"k\.\.128"):
        ev.evaluate(torch.zeros(2, 3), feat, [0, 1], (1, 5), diversity=0.5, pool=4)
    with pytest.raises(ValueError, match="diversity"):
        ev.evaluate(torch.zeros(2, 3), feat, [0, 1], (1, 5), pool=8)


def test_train_dcue_options():
    import train_dcue
    base = ["--synthetic", "--recommend-k", "5", "--recommend-out", "r.csv", "--eval-k", "1,5", "--eval-out", "m.json"]
    a = train_dcue.parse(base)
    assert a.recommend_diversity is None and a.recommend_pool is None and a.eval_diversity is None and not a.eval_ild
    a = train_dcue.parse(base + ["--recommend-diversity", "0.7", "--recommend-pool", "20", "--eval-ild",
                                 "--eval-diversity", "0.5"])
    assert (a.recommend_diversity, a.recommend_pool, a.eval_diversity, a.eval_ild) == (0.7, 20, 0.5, True)
    for bad in (["--synthetic", "--recommend-diversity", "0.5"], ["--synthetic", "--eval-ild"],
                base + ["--recommend-pool", "20"], base + ["--recommend-diversity", "1.5"],
                base + ["--eval-diversity", "-0.1"]):
        with pytest.raises(SystemExit):
            train_dcue.parse(bad)


# ------------------------------------------------------------------------------- compiled kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_diversify_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("diversify.hip", tmp_path)
    for kern in ("k_list_mmr", "k_list_ild", "k_list_ild_mean"):
        found = {k: v for k, v in res.items() if "%d%sE" % (len(kern), kern) in k}  # the Itanium-mangled name
        assert len(found) == 1, (kern, sorted(res))
        for k, v in found.items():
            assert v.get("ScratchSize", -1) == 0, (k, v)


def lds_bytes(pool, d):
    """csrc/diversify.h div_lds_bytes, mirrored: the row tile [p16][chunk + 4] and the Gram [p16][p16 + 1]
    share one region; colsum, idx, rel, inv, order and the flag words follow."""
    p16, dp = (pool + 15) // 16 * 16, (d + 15) // 16 * 16
    chunk = min(dp, 128)
    tile = max(p16 * (chunk + 4), p16 * (p16 + 1))
    return (tile + 3) // 4 * 4 * 4 + 128 * 8 + 4 * 128 * 4 + 16


HOST_CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler")
def test_lds_sizes_match_the_header_and_fit(tmp_path):
    """The kernels' dynamic LDS as csrc/diversify.h computes it (the header compiled alone, on the host)
    equals the mirror above at every pool / d regime, and the worst case fits a CU's 160 KiB -- twice."""
    shapes = [(p, d) for p in (1, 2, 16, 17, 63, 64, 65, 100, 128) for d in (1, 4, 16, 17, 100, 128, 129, 256)]
    src = tmp_path / "lds.cpp"
    src.write_text('#include <cstdio>\n#include "diversify.h"\nint main() {\n'
                   + "".join('  std::printf("%%zu\\n", dcue::div_lds_bytes(%d, %d));\n' % s for s in shapes)
                   + "  return 0;\n}\n")
    exe = tmp_path / "lds"
    subprocess.run([HOST_CXX, "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True,
                   timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [lds_bytes(*s) for s in shapes]
    assert lds_bytes(128, 256) == 128 * 132 * 4 + 3088 == 70672 and 2 * lds_bytes(128, 256) <= 160 * 1024
    assert lds_bytes(16, 16) == 16 * 20 * 4 + 3088  # small pools do not pay for the large one
