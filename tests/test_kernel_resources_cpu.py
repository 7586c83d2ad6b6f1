"""Register budget of the conv-1 forward (CPU: hipcc cross-compiles gfx950 here).

The split-f16 row-GEMM forward (csrc/conv_rows.h) runs two 512-thread workgroups per CU only while
it needs <= 128 VGPRs: one more register halves its occupancy, and the catalogue conv-1 forward --
the largest launch of a catalogue step -- went 92 -> 120 us when a slab-fill change took it to 156
(round 3). This compiles conv_fwd.hip with the kernel-resource remarks and holds every non-DEEP
split-f16 conv-1 instance (the ones launched with several workgroups per CU) to 128 VGPRs and no
scratch.

The evaluator's kernels (csrc/rank.hip) share their LDS sort with top-K (csrc/rank_sort.h); none of
them may spill.
"""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_conv1_forward_fits_two_workgroups_per_cu(tmp_path):
    res = kernel_resources("conv_fwd.hip", tmp_path)
    # k_conv_rows<MODE 0, SRC_TRACK_F16 (0), KC 128, ..., DEEP false, F16 true>
    conv1 = {k: v for k, v in res.items() if "k_conv_rowsILi0ELi0ELi128E" in k and k.endswith("Lb0ELb1EEEvNS_8RowsArgsE")}
    assert conv1, "no split-f16 conv-1 forward instance found"
    for k, v in conv1.items():
        assert v.get("VGPRs", 999) <= 128 and v.get("ScratchSize", 0) == 0, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rank_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("rank.hip", tmp_path)
    for kern in ("k_rank_normalize", "k_rank_scores", "k_rank_thresholds", "k_rank_hist", "k_rank_finalize",
                 "k_repeat_mean"):
        found = {k: v for k, v in res.items() if kern in k}
        assert len(found) == 1, (kern, sorted(res))
    for k, v in res.items():
        assert v.get("ScratchSize", -1) == 0, (k, v)
