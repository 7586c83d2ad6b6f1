"""The plan step's device-side cross-queue edges: the step-start signal,
the dgrad 4 / dgrad 3 fork signals with their one-wave relays, and the late Adam's relay.

They replace HIP event edges and change no arithmetic, so every run here is compared bit for bit:
the default mode against DCUE_XQ_WAIT=event and against each group of edges switched back to events
on its own (DCUE_XQ_START=0, DCUE_XQ_FORK=0, DCUE_XQ_LATE=0; child processes: the variables are read
once at load),
runs with 5 ms spins ahead of the producers and consumers of the signal words against the undelayed
run, and steps whose batch reaches reused device buffers only behind a 5 ms sleep on the caller's
stream against steps from fresh tensors. No test makes a wait give up: the fail word stays 0.

Shapes are tests/race_worker.py's (H = d = 64, E = 48, 40 users, 60 tracks, B = 16, N = 5, 5 steps,
flush_every 3) unless a case says otherwise."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DELAY_US = 5000
# the new sites, and the existing ones whose work now feeds or consumes a signal word
SITES = ["dgrad_4", "dgrad_3", "wgrad_hi", "wgrad_2", "user_bwd", "late_adam", "prologue"]
MODE_CASES = ["bn", "cat", "text", "small", "nonext"]
GROUPS = ["START", "FORK", "LATE"]
GROUP_CASES = ["bn", "text"]
# The library's launches over each MODE_CASES run (5 steps), measured at commit 3f6b92b, the parent of
# the change that split the step schedule out of capi.hip: a change to the schedule's code that is
# meant to leave each stream's sequence alone leaves these alone.
LAUNCHES = {"bn": 177, "cat": 176, "text": 211, "small": 177, "nonext": 176}
LAUNCHES_EVENT = {"bn": 137, "cat": 136, "text": 167, "small": 137, "nonext": 136}


def _same(a, b, what):
    import step_signal_worker as W
    assert W.finite(a), "%s: non-finite" % what
    for k in ("loss", "P", "emb"):
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


@pytest.fixture(scope="module")
def default_runs():
    """The default mode's runs of the mode comparison, made once in this process."""
    import step_signal_worker as W
    return {n: W.run(**W.CASES[n]) for n in MODE_CASES}


def _child_runs(out, cases, **env):
    """step_signal_worker's runs of `cases` in one child process with `env` set; the fail word is 0."""
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "step_signal_worker.py"), out,
                        ",".join(cases)], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=200)
    assert p.returncode == 0, p.stdout[-3000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["fail_flags"] == 0, info
    return info, torch.load(out)


@pytest.fixture(scope="module")
def event_runs(tmp_path_factory):
    """The same runs with every edge a HIP event edge (DCUE_XQ_WAIT=event), in one child process."""
    info, runs = _child_runs(str(tmp_path_factory.mktemp("xq") / "event.pt"), MODE_CASES, DCUE_XQ_WAIT="event")
    assert info["xq_wait"] == "event", info
    return runs


@pytest.mark.parametrize("case", MODE_CASES)
def test_modes_agree_bit_for_bit(case, default_runs, event_runs):
    _same(default_runs[case], event_runs[case], "%s: device signals against event edges" % case)


@pytest.mark.parametrize("group", GROUPS)
def test_each_group_as_events_agrees_bit_for_bit(group, default_runs, tmp_path):
    """One group of edges back on HIP events, the other two on signals: the branches that
    DCUE_XQ_START=0, DCUE_XQ_FORK=0 and DCUE_XQ_LATE=0 select, one child process per group."""
    info, runs = _child_runs(str(tmp_path / "group.pt"), GROUP_CASES, **{"DCUE_XQ_" + group: "0"})
    assert info["xq_groups"] == {g: "0" if g == group else "" for g in GROUPS} and info["xq_wait"] == "", info
    for case in GROUP_CASES:
        _same(runs[case], default_runs[case], "%s: DCUE_XQ_%s=0 against device signals" % (case, group))


@pytest.mark.parametrize("case", MODE_CASES)
def test_launch_counts_are_the_recorded_ones(case, default_runs, event_runs):
    assert default_runs[case]["launches"] == LAUNCHES[case]
    assert event_runs[case]["launches"] == LAUNCHES_EVENT[case]


def test_default_mode_runs_the_relays(default_runs, event_runs):
    """The comparison above has two sides: the default mode launches the relays and signals that the
    event mode does not (k_wait_signals ahead of the layer 3-5 and layer-2 weight gradients, the user
    tower's backward and the late Adam; k_signal after the two weight-gradient reduces)."""
    from dcrecommend import _native as nat
    assert default_runs["bn"]["launches"] > event_runs["bn"]["launches"]
    assert nat.debug_fail_flags() == 0


@pytest.mark.parametrize("inbatch", [True, False], ids=["inbatch", "catalogue"])
def test_delays_leave_the_bits_unchanged(inbatch, default_runs):
    import step_signal_worker as W
    from dcrecommend import _native as nat
    base = default_runs["bn" if inbatch else "cat"]
    for site in SITES:
        _same(W.run("bn", {site: DELAY_US}, inbatch=inbatch), base,
              "%s plan, delay at %s" % ("in-batch" if inbatch else "catalogue", site))
    assert nat.debug_fail_flags() == 0


@pytest.mark.parametrize("set_next", [True, False], ids=["lookahead", "no_lookahead"])
def test_step_start_orders_the_staged_batch(set_next, default_runs):
    """Each step's users (and items) reach the reused buffers behind a 5 ms sleep on the caller's
    stream: a user tower or prologue that did not wait for the step's start -- the start signal with
    the lookahead, the start event without it -- would read the previous batch."""
    import step_signal_worker as W
    from dcrecommend import _native as nat
    base = default_runs["bn" if set_next else "nonext"]
    _same(W.run("bn", set_next=set_next, staged=True), base, "staged batch, set_next=%s" % set_next)
    assert nat.debug_fail_flags() == 0
