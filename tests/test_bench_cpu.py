"""Host-side pieces of bench.py that need no GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_fail_flag_failures():
    import bench
    assert bench.fail_flag_failures(0) == []
    f = bench.fail_flag_failures(1)
    assert len(f) == 1 and "bit 0" in f[0]
    f = bench.fail_flag_failures(2)
    assert len(f) == 1 and "bit 1" in f[0]
    f = bench.fail_flag_failures(5)
    assert len(f) == 2 and "0x4" in f[1]


def test_plain_run_is_the_default(monkeypatch):
    """--full and --dump-outputs are off unless asked for; --steps is taken as given."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere"
