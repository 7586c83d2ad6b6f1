"""Host side of the top-K ranking metrics (include/dcue.h dcue_topk_metrics / dcue_topk_metrics_mean,
added under ABI 17), no GPU needed: the numpy reference against the header's worked example and hand
cases, the constants and symbols of header, binding and library, every bad-argument return (both
calls validate on the host before their first device call), the Python argument checks and the
compiled kernels' scratch use."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import topk_metrics_reference as R
from conftest import ROOT
from kernel_resources import HIPCC, kernel_resources

OK, INVALID = 0, 1


# ------------------------------------------------------------------------------- the reference
def test_reference_worked_example():
    got = R.query_metrics([7, 1, 3, 5], 4, {3, 7, 9}, [1, 2, 4])
    want = np.array([[1.0, 1 / 3, 1.0, 1.0, 1.0, 1.0],
                     [0.5, 1 / 3, 0.6131471927654584, 0.5, 1.0, 1.0],
                     [0.5, 2 / 3, 0.7039180890341347, 0.5555555555555556, 1.0, 1.0]])
    assert np.abs(got - want).max() <= 1e-15
    assert abs(got[1, R.NDCG] - 1 / (1 + 1 / math.log2(3))) <= 1e-15
    assert abs(got[2, R.NDCG] - 1.5 / 2.1309297535714573) <= 1e-15
    assert abs(got[2, R.MAP] - (1 + 2 / 3) / 3) <= 1e-15


def test_reference_all_hits():
    got = R.query_metrics([4, 2, 9], 3, {2, 4, 9}, [1, 3])
    assert np.array_equal(got, np.array([[1, 1 / 3, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]], np.float64))


def test_reference_no_hit():
    got = R.query_metrics([4, 2, 9], 3, {1, 5}, [1, 3])
    assert np.array_equal(got, np.zeros((2, 6)))


def test_reference_truth_larger_than_cutoff():
    # t = 5 > cutoff 2: recall is bounded by 2/5, the ideal list has 2 hits, MAP divides by 2
    got = R.query_metrics([8, 1, 3, 5], 4, {1, 3, 5, 7, 9}, [2])
    idcg = 1 + 1 / math.log2(3)
    want = [0.5, 1 / 5, (1 / math.log2(3)) / idcg, (1 / 2) / 2, 0.5, 1.0]
    assert np.abs(got[0] - want).max() <= 1e-15


def test_reference_list_shorter_than_cutoff():
    # c = 2 < cutoff 4: precision still divides by 4; the entries past c are not looked at
    got = R.query_metrics([3, 6, 7, 7], 2, {3, 7}, [4])
    idcg = 1 + 1 / math.log2(3)
    want = [1 / 4, 1 / 2, 1 / idcg, 1 / 2, 1.0, 1.0]
    assert np.abs(got[0] - want).max() <= 1e-15


def test_reference_flags_exposure_coverage_and_means():
    idx = np.array([[7, 1, 3, 5], [2, 2, -1, -1], [9, 0, 1, -1], [10, 1, 2, 3], [1, -5, 0, 0]])
    count = np.array([4, 1, 3, 4, 1])
    ptr = np.array([0, 3, 3, 5])
    tidx = np.array([3, 7, 9, 0, 2])
    queries = [0, 1, 2, 2, 2]  # row 1 has no truth; the fourth list holds n_cand; the -5 lies past count
    expo = np.zeros((2, 10), np.int64)
    per, flags = R.metrics(idx, count, queries, ptr, tidx, [1, 4], 10, expo)
    assert flags.tolist() == [0, 1, 0, 2, 0]
    assert np.all(per[1] == 0) and np.all(per[3] == 0)
    assert expo[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 1]
    assert expo[1].tolist() == [1, 2, 0, 1, 0, 1, 0, 0, 0, 0]
    mask = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 1], np.uint8)
    assert R.coverage(expo, mask, 10).tolist() == [3 / 8, 6 / 8]
    assert R.coverage(expo, None, 10).tolist() == [0.3, 0.6]
    mean, n = R.means(per, flags)
    assert n == 3 and np.array_equal(mean, (per[0] + per[2] + per[4]) / 3)
    assert R.means(per[[1, 3]], flags[[1, 3]])[1] == 0


# ------------------------------------------------------------------------------- the surface
def test_header_binding_and_library_agree():
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1))

    assert define("DCUE_TOPK_METRICS_MAX_CUTOFFS") == nat.TOPK_METRICS_MAX_CUTOFFS == 8
    assert define("DCUE_TOPK_N_METRICS") == nat.TOPK_N_METRICS == R.N_METRICS == 6
    for slot, name in enumerate(nat.TOPK_METRIC_NAMES):
        assert define("DCUE_TOPK_METRIC_" + name.upper()) == slot
    assert nat.TOPK_METRIC_NAMES == R.NAMES
    assert define("DCUE_TOPK_FLAG_NO_TRUTH") == nat.TOPK_FLAG_NO_TRUTH == R.FLAG_NO_TRUTH
    assert define("DCUE_TOPK_FLAG_BAD_INDEX") == nat.TOPK_FLAG_BAD_INDEX == R.FLAG_BAD_INDEX
    for sym in ("dcue_topk_metrics", "dcue_topk_metrics_mean"):
        assert re.search(r"\bint %s\(" % sym, hdr) and sym in nat._SIGS
        assert getattr(nat.lib(), sym).argtypes == nat._SIGS[sym][0]
    assert define("DCUE_ABI_VERSION") == 17
    assert nat.ABI_VERSION == 17 and nat.lib().dcue_abi_version() == 17


# ------------------------------------------------------------------------------- bad arguments
def _p():
    """A never-dereferenced non-null address: every case returns before a device call."""
    return ctypes.c_void_p(0x1000)


def _metrics(cutoffs=(1, 5, 10), **over):
    from dcrecommend import _native as nat
    cut = (ctypes.c_int32 * max(len(cutoffs), 1))(*cutoffs)
    a = dict(idx=_p(), count=_p(), n_queries=4, k=10, queries=_p(), truth_ptr=_p(), truth_idx=_p(), n_query_rows=10,
             n_cand=1000, cutoffs_host=ctypes.cast(cut, ctypes.c_void_p), n_cutoffs=len(cutoffs), out_metrics=_p(),
             out_flags=_p(), exposure=_p(), stream=None)
    a.update(over)
    order = ("idx", "count", "n_queries", "k", "queries", "truth_ptr", "truth_idx", "n_query_rows", "n_cand",
             "cutoffs_host", "n_cutoffs", "out_metrics", "out_flags", "exposure", "stream")
    return nat.lib().dcue_topk_metrics(*[a[n] for n in order])


def _mean(**over):
    from dcrecommend import _native as nat
    a = dict(metrics=_p(), flags=_p(), n_queries=4, n_cutoffs=3, exposure=_p(), cand_mask=_p(), n_cand=1000,
             out_mean=_p(), out_coverage=_p(), out_n_evaluated=_p(), stream=None)
    a.update(over)
    order = ("metrics", "flags", "n_queries", "n_cutoffs", "exposure", "cand_mask", "n_cand", "out_mean",
             "out_coverage", "out_n_evaluated", "stream")
    return nat.lib().dcue_topk_metrics_mean(*[a[n] for n in order])


@pytest.mark.parametrize("name", ["idx", "count", "queries", "truth_ptr", "truth_idx", "cutoffs_host", "out_metrics",
                                  "out_flags"])
def test_metrics_null_pointer_is_invalid(name):
    assert _metrics(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(k=0), dict(k=129), dict(n_cutoffs=0), dict(n_cutoffs=9), dict(n_cand=0),
                                  dict(n_cand=-3), dict(n_queries=-1), dict(n_query_rows=0)])
def test_metrics_bad_argument_is_invalid(over):
    assert _metrics(**over) == INVALID


@pytest.mark.parametrize("cutoffs", [(0, 5), (-1,), (5, 5), (5, 3), (1, 5, 11), (11,), (1, 2, 3, 3)])
def test_metrics_bad_cutoffs_are_invalid(cutoffs):
    assert _metrics(cutoffs=cutoffs) == INVALID


def test_metrics_nothing_to_do_is_ok():
    assert _metrics(n_queries=0) == OK
    assert _metrics(n_queries=0, exposure=None, cutoffs=(10,)) == OK
    assert _metrics(n_queries=0, k=128, cutoffs=(1, 2, 3, 4, 5, 6, 7, 128)) == OK


@pytest.mark.parametrize("name", ["metrics", "flags", "out_mean", "out_n_evaluated"])
def test_mean_null_pointer_is_invalid(name):
    assert _mean(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(n_cutoffs=0), dict(n_cutoffs=9), dict(n_cand=0), dict(n_queries=-1),
                                  dict(exposure=None), dict(out_coverage=None)])
def test_mean_bad_argument_is_invalid(over):
    """(exposure and out_coverage are null together or not at all)"""
    assert _mean(**over) == INVALID


# ------------------------------------------------------------------------------- Python arguments
def test_cutoff_checks_name_the_limit():
    from dcrecommend.nn import rank
    assert rank.check_cutoffs((100, 10, 10, 50)) == [10, 50, 100]
    with pytest.raises(ValueError, match="at least 1"):
        rank.check_cutoffs(())
    with pytest.raises(ValueError, match=r"1\.\.128"):
        rank.check_cutoffs((0, 10))
    with pytest.raises(ValueError, match=r"1\.\.128"):
        rank.check_cutoffs((10, 129))
    with pytest.raises(ValueError, match="at most 8"):
        rank.check_cutoffs(range(1, 10))
    assert rank.check_cutoffs(range(1, 9)) == list(range(1, 9))


def test_topk_metrics_argument_checks():
    import torch
    from dcrecommend.nn import rank
    ptr, idx = np.array([0, 2, 2, 3]), np.array([1, 4, 0])
    with pytest.raises(ValueError, match="n_cand"):
        rank.TopKMetrics(ptr, idx, "cpu")
    with pytest.raises(ValueError, match="CSR"):
        rank.TopKMetrics(np.array([0, 2, 5]), idx, "cpu", n_cand=6)
    with pytest.raises(ValueError, match="rows"):
        rank.TopKMetrics(ptr, idx, "cpu", excl_ptr=np.array([0, 1]), excl_idx=np.array([2]), n_cand=6)
    ev = rank.TopKMetrics(ptr, idx, "cpu", n_cand=6)
    feat = torch.zeros(3, 4)
    for ks, match in (((), "at least 1"), ((0,), r"1\.\.128"), ((129,), r"1\.\.128"), (range(1, 10), "at most 8")):
        with pytest.raises(ValueError, match=match):
            ev.evaluate(feat, torch.zeros(6, 4), [0, 1], ks)
        with pytest.raises(ValueError, match=match):
            ev.metrics_raw(torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), [0, 1], ks)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path exists
        ev.metrics_raw(torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), [0, 1], (1, 2))


def test_evaluate_topk_argument_checks():
    from dcrecommend.nn.dcue import DCUE
    tr = DCUE(feature_dim=8, conv_hidden=8, batch_size=4, device="cpu")
    for ks, match in (((), "at least 1"), ((0, 10), r"1\.\.128"), ((10, 200), r"1\.\.128"),
                      (range(1, 10), "at most 8")):
        with pytest.raises(ValueError, match=match):
            tr.evaluate_topk(ks=ks)
    with pytest.raises(RuntimeError, match="no factors"):
        tr.evaluate_topk(ks=(1, 5))


# ------------------------------------------------------------------------------- compiled kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_topk_metrics_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("topk_metrics.hip", tmp_path)
    for kern in ("k_topk_metrics", "k_topk_metrics_table", "k_topk_metrics_mean"):
        found = {k: v for k, v in res.items() if "%d%sE" % (len(kern), kern) in k}  # the Itanium-mangled name
        assert len(found) == 1, (kern, sorted(res))
        for k, v in found.items():
            assert v.get("ScratchSize", -1) == 0, (k, v)
