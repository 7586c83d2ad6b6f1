"""Worker for tests/test_gpu_shapes.py::test_forced_tilings_against_oracle: the (5, 12) and (43, 2)
catalogue cases with the row tiling the parent forced (DCUE_ROWS_TW, read once per process), under
the same checks as the planner's own choice."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import launch_shape_cases as C
    import test_gpu_shapes as T
    from dcrecommend import _native as nat
    tw = int(os.environ["DCUE_ROWS_TW"])
    for case in T.FORCED_CASES:
        # the report follows the forced tiling wherever its slab fits: it names what these launches do
        got = sorted({v[0] for kind in ("fwd", "dgrad") for v in C.shape_of(nat, case)[kind].values()})
        assert tw in got, "DCUE_ROWS_TW=%d did not take: TW %s" % (tw, got)
        T.run_case(case)
    print("forced tilings ok: TW %d" % tw)
    return 0


if __name__ == "__main__":
    sys.exit(main())
