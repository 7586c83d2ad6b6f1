"""Worker for tests/test_gpu_text_shapes.py::test_first_maximum_across_position_parts: the exact-tie
case with the text forward's A/B knobs as the parent set them (read once per process)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import test_gpu_text_shapes as S
    T = int(sys.argv[1])
    S.run_ties(T)
    print("text ties ok: T %d parts %s" % (T, os.environ.get("DCUE_TEXT_PARTS", "1")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
