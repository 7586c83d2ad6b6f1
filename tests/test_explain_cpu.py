"""Host side of explained lists (include/dcue.h dcue_list_explain, added under ABI 17), no GPU needed:
the numpy reference against a brute-force restatement and hand cases, the constants and symbols of
header, binding and library, every bad-argument return (the call validates on the host before its first
device call), the workspace formula, the LDS layout header compiled alone, the compiled kernel's scratch
and LDS use, and the Python argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import explain_reference as R
from conftest import ROOT
from kernel_resources import HIPCC, PKG, kernel_resources

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4  # dcue_status


# ------------------------------------------------------------------------------- the reference
def _random_case(seed, n_cand=60, d=6, n_rows=7, k=9):
    rs = np.random.RandomState(seed)
    feat = rs.randn(n_cand, d).astype(np.float32)
    rows = [np.sort(rs.choice(n_cand, rs.randint(0, 25), replace=False)) for _ in range(n_rows)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    mask = (rs.rand(n_cand) < 0.7).astype(np.uint8)
    lists = np.stack([rs.choice(n_cand, k, replace=False) for _ in range(n_rows)]).astype(np.int32)
    counts = rs.randint(0, k + 1, n_rows).astype(np.int32)
    return feat, ptr, idx, mask, lists, counts


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("masked", [False, True])
def test_reference_matches_brute_force(seed, masked):
    feat, ptr, idx, mask, lists, counts = _random_case(seed)
    mask = mask if masked else None
    for m in (1, 3, 8):
        for u in range(len(lists)):
            why_idx, why_sim, flags = R.explain_list(lists[u], counts[u], u, ptr, idx, feat, m, mask)
            H, _ = R.history(u, ptr, idx, len(feat), mask)
            assert flags == (R.FLAG_NO_HISTORY if len(H) == 0 else 0)
            brute = R.explain_brute(lists[u], counts[u], u, ptr, idx, feat, m, mask)
            assert len(brute) == counts[u]
            for j, pairs in enumerate(brute):
                n = len(pairs) if len(H) else 0
                assert why_idx[j, :n].tolist() == [p[0] for p in pairs[:n]]
                assert np.abs(why_sim[j, :n] - [p[1] for p in pairs[:n]]).max(initial=0) <= 1e-15
                assert np.all(why_idx[j, n:] == -1) and np.all(np.isneginf(why_sim[j, n:]))
            assert np.all(why_idx[counts[u]:] == -1) and np.all(np.isneginf(why_sim[counts[u]:]))


FEAT = np.array([[1, 0], [2, 0], [0, 3], [1, 1], [0, 0], [-1, 0], [5, 0]], np.float32)


def test_reference_ties_go_to_the_lower_index():
    # rows 0, 1 and 6 are the same direction: cosine 1 with pick 0, three ways
    ptr, idx = np.array([0, 4]), np.array([1, 2, 5, 6], np.int32)
    why_idx, why_sim, flags = R.explain_list([0], 1, 0, ptr, idx, FEAT, 3)
    assert flags == 0 and why_idx[0].tolist() == [1, 6, 2] and why_sim[0].tolist() == [1.0, 1.0, 0.0]
    assert R.explain_list([0], 1, 0, ptr, idx, FEAT, 4)[0][0].tolist() == [1, 6, 2, 5]


def test_reference_short_history_pads():
    ptr, idx = np.array([0, 2]), np.array([2, 5], np.int32)
    why_idx, why_sim, flags = R.explain_list([0, 3], 2, 0, ptr, idx, FEAT, 4)
    assert flags == 0 and why_idx[0].tolist() == [2, 5, -1, -1] and why_sim[0].tolist() == [0.0, -1.0, -np.inf, -np.inf]
    assert why_idx[1].tolist() == [2, 5, -1, -1]


def test_reference_masked_entry_never_appears():
    ptr, idx = np.array([0, 3]), np.array([1, 2, 6], np.int32)
    mask = np.array([1, 0, 1, 1, 1, 1, 1], np.uint8)
    why_idx, _, flags = R.explain_list([0], 1, 0, ptr, idx, FEAT, 8, mask)
    assert flags == 0 and why_idx[0].tolist() == [6, 2] + [-1] * 6


def test_reference_empty_or_all_masked_row_sets_bit_0():
    ptr, idx = np.array([0, 0, 2]), np.array([1, 2], np.int32)
    why_idx, why_sim, flags = R.explain_list([0, 3], 2, 0, ptr, idx, FEAT, 2)
    assert flags == R.FLAG_NO_HISTORY and np.all(why_idx == -1) and np.all(np.isneginf(why_sim))
    mask = np.array([1, 0, 0, 1, 1, 1, 1], np.uint8)
    why_idx, _, flags = R.explain_list([0, 3], 2, 1, ptr, idx, FEAT, 2, mask)
    assert flags == R.FLAG_NO_HISTORY and np.all(why_idx == -1)
    assert R.explain_list([0, 3], 0, 0, ptr, idx, FEAT, 2)[2] == R.FLAG_NO_HISTORY  # an empty list still says so


def test_reference_pick_in_its_own_history_comes_first():
    ptr, idx = np.array([0, 3]), np.array([2, 3, 5], np.int32)
    why_idx, why_sim, flags = R.explain_list([3], 1, 0, ptr, idx, FEAT, 3)
    assert flags == 0 and why_idx[0, 0] == 3 and abs(why_sim[0, 0] - 1.0) <= 1e-15


def test_reference_flags():
    ptr, idx = np.array([0, 2, 4]), np.array([1, 2, 1, 9], np.int32)
    assert R.explain_list([0, 9], 2, 0, ptr, idx, FEAT, 2)[2] == R.FLAG_BAD_INDEX  # a list entry
    assert R.explain_list([0, 9], 1, 0, ptr, idx, FEAT, 2)[2] == 0  # past count: never read
    assert R.explain_list([0], 1, 1, ptr, idx, FEAT, 2)[2] == R.FLAG_BAD_INDEX  # a history entry
    assert R.explain_list([0], 1, 2, ptr, idx, FEAT, 2)[2] == R.FLAG_BAD_INDEX  # the query row
    assert R.explain_list([0], 1, -1, ptr, idx, FEAT, 2)[2] == R.FLAG_BAD_INDEX
    bad = FEAT.copy()
    bad[2, 0] = np.nan
    why_idx, _, flags = R.explain_list([0, 2], 2, 0, ptr, idx, bad, 2)
    assert flags == R.FLAG_NONFINITE and why_idx[0].tolist() == [1, -1] and why_idx[1].tolist() == [-1, -1]
    # a zero row has similarity 0 to everything
    why_idx, why_sim, flags = R.explain_list([4], 1, 0, ptr, idx, FEAT, 2)
    assert flags == 0 and why_idx[0].tolist() == [1, 2] and why_sim[0].tolist() == [0.0, 0.0]
    why_idx, why_sim, flags = R.explain([[0, 1], [0, 9]], [5, 2], [0, 0], ptr, idx, FEAT, 1)  # count clamped to k
    assert flags.tolist() == [0, R.FLAG_BAD_INDEX] and why_idx.shape == (2, 2, 1) and why_idx[0, :, 0].tolist() == [1, 1]


def test_tolerant_check_rejects_a_wrong_reason():
    feat, ptr, idx, _, lists, _ = _random_case(3)
    u = int(np.argmax(np.diff(ptr)))
    why_idx, why_sim, _ = R.explain_list(lists[u], 9, u, ptr, idx, feat, 3)
    tol = (16 + 8) * 2.0 ** -24
    R.check_tolerant(why_idx, why_sim.astype(np.float32), lists[u], 9, u, ptr, idx, feat, 3, tol)
    why_idx[2, 0] = why_idx[2, 2]
    with pytest.raises(AssertionError):
        R.check_tolerant(why_idx, why_sim.astype(np.float32), lists[u], 9, u, ptr, idx, feat, 3, tol)


# ------------------------------------------------------------------------------- the surface
def test_header_binding_and_library_agree():
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1))

    assert define("DCUE_EXPLAIN_MAX_REASONS") == nat.EXPLAIN_MAX_REASONS == R.MAX_REASONS == 8
    assert define("DCUE_EXPLAIN_FLAG_NO_HISTORY") == nat.EXPLAIN_FLAG_NO_HISTORY == R.FLAG_NO_HISTORY == 1
    assert define("DCUE_LIST_FLAG_BAD_INDEX") == nat.LIST_FLAG_BAD_INDEX == R.FLAG_BAD_INDEX == 2
    assert define("DCUE_LIST_FLAG_NONFINITE") == nat.LIST_FLAG_NONFINITE == R.FLAG_NONFINITE == 4
    for sym in ("dcue_list_explain_workspace_bytes", "dcue_list_explain"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in nat._SIGS
        assert getattr(nat.lib(), sym).argtypes == nat._SIGS[sym][0]
    assert define("DCUE_ABI_VERSION") == 17
    assert nat.ABI_VERSION == 17 and nat.lib().dcue_abi_version() == 17


# ------------------------------------------------------------------------------- bad arguments
def _p():
    """A never-dereferenced non-null address: every case returns before a device call."""
    return ctypes.c_void_p(0x1000)


ORDER = ("idx", "count", "n_lists", "k", "queries", "hist_ptr", "hist_idx", "n_query_rows", "hist_mask", "cand_feat",
         "n_cand", "d", "m", "ws", "ws_bytes", "out_idx", "out_sim", "out_flags", "stream")


def _explain(**over):
    from dcrecommend import _native as nat
    a = dict(idx=_p(), count=_p(), n_lists=0, k=10, queries=_p(), hist_ptr=_p(), hist_idx=_p(), n_query_rows=50,
             hist_mask=None, cand_feat=_p(), n_cand=1000, d=100, m=3, ws=_p(), ws_bytes=1000 * 112 * 4, out_idx=_p(),
             out_sim=_p(), out_flags=_p(), stream=None)
    a.update(over)
    return nat.lib().dcue_list_explain(*[a[n] for n in ORDER])


def test_nothing_to_do_is_ok():
    assert _explain() == OK and _explain(hist_mask=_p()) == OK
    assert _explain(k=128, m=8, d=256, ws_bytes=1000 * 256 * 4) == OK and _explain(k=1, m=1, d=1) == OK


@pytest.mark.parametrize("name", ["idx", "count", "queries", "hist_ptr", "hist_idx", "cand_feat", "out_idx", "out_sim",
                                  "out_flags"])
def test_null_pointer_is_invalid(name):
    assert _explain(**{name: None}) == INVALID
    assert _explain(n_lists=3, **{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(m=0), dict(m=9), dict(m=-1), dict(n_cand=0),
                                  dict(n_cand=-3), dict(d=0), dict(n_query_rows=0), dict(n_query_rows=-1),
                                  dict(n_lists=-1)])
def test_bad_argument_is_invalid(over):
    assert _explain(**over) == INVALID
    assert _explain(**dict(dict(n_lists=3), **over)) == INVALID


@pytest.mark.parametrize("over", [dict(d=257), dict(n_cand=2 ** 31 - 64)])
def test_unsupported_sizes(over):
    assert _explain(ws_bytes=2 ** 62, **over) == UNSUPPORTED
    assert _explain(n_lists=3, ws_bytes=2 ** 62, **over) == UNSUPPORTED


def test_workspace_too_small_or_null():
    assert _explain(ws_bytes=1000 * 112 * 4 - 1) == WORKSPACE and _explain(n_lists=3, ws_bytes=0) == WORKSPACE
    assert _explain(ws=None) == WORKSPACE and _explain(n_lists=3, ws=None) == WORKSPACE


def test_workspace_bytes_is_a_host_computation():
    """The workspace holds the candidate table's unit rows: n_cand * rank_dp(d) floats."""
    from dcrecommend import _native as nat
    fn = nat.lib().dcue_list_explain_workspace_bytes
    n = ctypes.c_size_t(12345)
    for n_cand, d in ((1, 1), (400, 4), (400, 17), (2000, 100), (200000, 128), (2 ** 31 - 65, 256)):
        assert fn(n_cand, d, 4096, 100, 3, ctypes.byref(n)) == OK and n.value == n_cand * ((d + 15) // 16 * 16) * 4
    assert fn(1000, 100, 0, 1, 1, ctypes.byref(n)) == OK and fn(1000, 100, 7, 128, 8, ctypes.byref(n)) == OK
    assert fn(1000, 100, 4, 10, 3, None) == INVALID
    for args in ((0, 16, 1, 10, 3), (10, 0, 1, 10, 3), (10, 16, -1, 10, 3), (10, 16, 1, 0, 3), (10, 16, 1, 129, 3),
                 (10, 16, 1, 10, 0), (10, 16, 1, 10, 9)):
        assert fn(*args, ctypes.byref(n)) == INVALID
    assert fn(10, 257, 1, 10, 3, ctypes.byref(n)) == UNSUPPORTED
    assert fn(2 ** 31 - 64, 16, 1, 10, 3, ctypes.byref(n)) == UNSUPPORTED


# ------------------------------------------------------------------------------- Python arguments
def test_python_argument_checks():
    import torch
    from dcrecommend.nn import rank
    assert rank.check_reasons(1) == 1 and rank.check_reasons(8) == 8
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match=r"1\.\.8"):
            rank.check_reasons(bad)
    ex = rank.Explain("cpu")
    idx, count = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    feat, ptr, hidx = torch.zeros(6, 3), np.array([0, 1, 2]), np.array([1, 4])
    with pytest.raises(ValueError, match=r"1\.\.8"):  # before any device work
        ex.explain_raw(idx, count, [0, 1], ptr, hidx, feat, 9)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path exists
        ex.explain_raw(idx, count, [0, 1], ptr, hidx, feat, 3)
    with pytest.raises(IndexError, match="query 7"):
        rank.check_explain_flags([5, 7], np.array([1, 2]))
    with pytest.raises(ValueError, match="Input contains NaN.*query 5"):
        rank.check_explain_flags([5, 7], np.array([4, 1]))
    rank.check_explain_flags([5, 7], np.array([0, 1]))  # no history: not an error


def test_trainers_check_reasons_first():
    from dcrecommend.dcbr.wrmf import WRMF
    from dcrecommend.nn.dcue import DCUE
    for cls in (DCUE, WRMF):
        for name in ("explain",) + (("explain_for",) if cls is DCUE else ()):
            with pytest.raises(ValueError, match=r"1\.\.8"):
                getattr(cls, name)(object.__new__(cls), ["u"], k=5, reasons=9)


def test_train_dcue_options():
    import train_dcue
    base = ["--synthetic", "--recommend-k", "5", "--recommend-out", "r.csv"]
    a = train_dcue.parse(base)
    assert a.recommend_reasons is None and a.reasons_out is None
    a = train_dcue.parse(base + ["--recommend-reasons", "3", "--reasons-out", "why.csv", "--recommend-diversity", "0.7",
                                 "--recommend-for", "new.csv"])
    assert (a.recommend_reasons, a.reasons_out, a.recommend_diversity, a.recommend_for) == (3, "why.csv", 0.7, "new.csv")
    for bad in (base + ["--recommend-reasons", "3"], base + ["--reasons-out", "why.csv"],
                ["--synthetic", "--recommend-reasons", "3", "--reasons-out", "why.csv"],
                base + ["--recommend-reasons", "9", "--reasons-out", "why.csv"],
                base + ["--recommend-reasons", "0", "--reasons-out", "why.csv"]):
        with pytest.raises(SystemExit):
            train_dcue.parse(bad)


# ------------------------------------------------------------------------------- compiled kernel
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_explain_kernel_uses_no_scratch_and_no_static_lds(tmp_path):
    """Zero scratch, and no LDS of its own: every byte is the dynamic allocation csrc/explain.h sizes."""
    res = kernel_resources("explain.hip", tmp_path)
    kern = "k_list_explain"
    found = {k: v for k, v in res.items() if "%d%sE" % (len(kern), kern) in k}  # the Itanium-mangled name
    assert len(found) == 1, sorted(res)
    for k, v in found.items():
        assert v.get("ScratchSize", -1) == 0, (k, v)
        assert v.get("LDS Size", -1) == 0, (k, v)


def lds_bytes(d):
    """csrc/explain.h exp_lds_bytes, mirrored: the list rows' and the history tile [64][dp + 4] floats each,
    the score tile [64][65] floats (the merge keys [4][8][64] of 8 bytes fit inside), the tile's candidates
    and the pass's list entries [64] words each, 4 words of flags."""
    dp = (d + 15) // 16 * 16
    return 2 * 64 * (dp + 4) * 4 + max(64 * 65 * 4, 64 * 4 * 8 * 8) + 64 * 4 + 64 * 4 + 16


HOST_CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler")
def test_lds_sizes_match_the_header_and_fit(tmp_path):
    """The kernel's dynamic LDS as csrc/explain.h computes it (the header compiled alone, on the host)
    equals the mirror above at every d regime, and the worst case fits a CU's 160 KiB."""
    ds = [1, 4, 16, 17, 100, 128, 129, 255, 256]
    src = tmp_path / "lds.cpp"
    src.write_text('#include <cstdio>\n#include "explain.h"\nint main() {\n'
                   + "".join('  std::printf("%%zu\\n", dcue::exp_lds_bytes(%d));\n' % d for d in ds)
                   + "  return 0;\n}\n")
    exe = tmp_path / "lds"
    subprocess.run([HOST_CXX, "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True,
                   timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [lds_bytes(d) for d in ds]
    assert lds_bytes(256) == 2 * 64 * 260 * 4 + 16640 + 528 == 150288 <= 160 * 1024
    assert lds_bytes(16) == 2 * 64 * 20 * 4 + 17168  # small d does not pay for the large one
