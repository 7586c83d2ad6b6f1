"""Frozen user-table rows (csrc/adam_replay.h "frozen rows", csrc/adam.hip) on the GPU:
freeze, skip, refresh, return, full flush, thaw and checkpoint, against the dense per-step sweep.

Reference: NativeAdam(defer_embedding=False), itself pinned bit for bit to torch's restatement by
tests/test_gpu_adam_exact.py. Bar: BIT-EXACT (torch.equal) losses, parameters, buffers and all four
moment tensors; no tolerance anywhere. Beside the values, the test reads the lazy optimizer's raw row
clocks (emb_step; bit 30 = frozen) and the 32-byte dcue_emb_log header (include/dcue.h: word 0
step_done, 1 flush_step, 5 frz_start, 6 frz_S, 7 frz_eps) between phases and asserts that each frozen
path provably ran -- reading them launches nothing in the library.

One deterministic, phased schedule (104 users, B = 8, flush_every = cap = 4, beta1 = 0.6 so that rows
freeze 50-80 idle steps after their gradient step instead of 300+):
  A   12 steps: step s takes users 8s..8s+7 (rows 0..95 one gradient step each, 96..103 none; one
      batch lists a user twice -- its left-out row is hot and gets its step in B);
  B   96 steps drawn from the hot rows 0..15 only; rows 16..95 sit idle and freeze (the freeze
      assertions also run 5/8 of the way, while rows are still crossing the bound);
      snapshot, freeze assertions, full flush + state equality;
  B'  9 hot steps, so that the frozen rows lag behind again and the returns below replay a non-empty
      recurrence (straight after a flush every row is current and a return replays nothing);
  C   return: 8 frozen rows; one frozen row twice among hot rows; never-touched rows 96..99;
  D   40 hot steps (>= 8 cap + cap): frozen rows fall 8 cap behind and are refreshed (m / v only);
      snapshot, refresh assertions, full flush + state equality;
  D'  9 hot steps, so that the thaw below has steps to replay;
  E   epoch change (lr x 20 | eps / 10 | betas -> (0.7, 0.99) | weight decay 1e-3 for 6 steps), or a
      state_dict / load_state_dict round trip of the lazy optimizer instead;
  F   102 hot steps (B's length + the ln 20 / ln(1 / 0.6) ~ 6 steps the 20 x larger S needs) to
      re-freeze under the new epoch, freeze assertions again, then return batches as in C;
  end eval-mode user features of all users, flush, full state equality.

Observed on the MI355X over the twelve cases (cold rows = 16..95; run with -s to print them):
  B, 5/8 of the way (step 72): 64-70 cold rows with moments frozen, 34-54 in the must-be-frozen set,
      16-18 rows in the must-not set -- the only snapshot with rows between the two sets;
  end of B (step 108): all 80 cold rows in the must-be-frozen set and frozen, 70-74 of them with
      non-zero moments (the other 6-10 took an exactly zero gradient in A: every hinge term of
      theirs inactive), 88 rows frozen in all (the 8 never-touched ones too), the 16 hot rows in the
      must-not set;
  C / F returns: the 8 rows and the doubled row frozen before their step and 9-30 steps behind;
  D: 61-65 cold frozen rows refreshed (skipped, then m / v only, bit kept);
  E: 75-76 frozen rows thawed (lr, eps, betas, wd); after the step 23-24 rows frozen again by its
      own slice under the new epoch (none under weight decay or in plans, whose slice comes a step late);
  end of F: all 80 cold rows in the must-be-frozen set and frozen again (weight decay variant: all
      80 with non-zero moments, the decay having given every row some);
  beta1 = 0.9, eps = 1e-4, idle phases of 320 steps: the same picture at steps 212 / 332 / 742
      (65, then 73 cold rows with moments frozen; 65 refreshed; 76 thawed).
  Each case takes 0.2-0.3 s (0.7 s at beta1 = 0.9).
"""
import collections
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_USERS, HOT, B, N, N_TRACKS, CAP = 104, 16, 8, 3, 48, 4
LR, EPS, WD_E = 1e-3, 1e-8, 1e-3
LEN_A, LEN_B, LEN_LAG, LEN_D, LEN_WD = 12, 96, 2 * CAP + 1, 8 * CAP + CAP + 4, 6
FROZEN = 1 << 30
MAX_LAG = 8 * CAP + CAP  # kFrzRefreshCaps x cap (adam.hip) + one round of the rolling slices
COLD = np.arange(HOT, LEN_A * B)


def _mt(seed):
    from dcrecommend import _native as nat
    st = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=DEV)
    nat.check(nat.lib().dcue_mt_seed(nat.ptr(st), seed, nat.stream_handle()), "mt_seed")
    return st


def _state(net, opt):
    out = {k: v.detach().clone() for k, v in net.state_dict().items()}
    st = opt._adam_state()
    for k in ("m", "v", "em", "ev"):
        out["adam." + k] = st[k].clone()
    return out


def _assert_equal_state(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        if not torch.equal(a[k], b[k]):
            bad = (a[k] != b[k]).nonzero()[0].tolist()
            raise AssertionError("%s: %s differs first at %s (dense %r, deferred %r), %d elements in all"
                                 % (where, k, bad, a[k][tuple(bad)].item(), b[k][tuple(bad)].item(),
                                    int((a[k] != b[k]).sum())))


Snap = collections.namedtuple("Snap", "T F start S eps bit low")


class _Run:
    """The dense run and the deferred one, stepped in lockstep on the same batches."""

    def __init__(self, E, use_plan, betas, eps):
        from dcrecommend.dcue.dcue import DCUENet
        from dcrecommend.optim import NativeAdam
        self.nets, self.opts = [], []
        for defer in (False, True):
            torch.manual_seed(3)
            net = DCUENet({"feature_dim": 32, "conv_hidden": 32, "user_embdim": E, "user_count": N_USERS,
                           "model_type": "truedcuemel1dbn"}).cuda().train()
            self.nets.append(net)
            self.opts.append(NativeAdam(net.parameters(), LR, betas, eps, 0.0, defer_embedding=defer,
                                        flush_every=CAP))
        self.gen = torch.Generator(device=DEV).manual_seed(7)
        self.rng = random.Random(11)
        self.tracks = torch.randn((N_TRACKS, 131, 128), generator=self.gen, device=DEV).half()
        self.plan = None
        if use_plan:
            from dcrecommend.dcue.plan import TrainPlan
            self.mts = [_mt(21), _mt(21)]
            self.neg = torch.zeros((B, N), dtype=torch.int32, device=DEV)
            self.plan = TrainPlan(self.nets[1], self.tracks, B, N, mt_state=self.mts[1], optimizer=self.opts[1])
        self.t = 0
        self.batches = {}  # Adam step -> the rows in its batch
        self.dense_hist = collections.deque(maxlen=CAP + 2)  # the dense table (p, m, v) after the last steps

    def group(self, **kw):  # the same param_group edit on both optimizers
        for opt in self.opts:
            opt.param_groups[0].update(kw)

    def hot(self):
        return [self.rng.randrange(HOT) for _ in range(B)]

    def step(self, users):
        from dcrecommend import _native as nat
        assert len(users) == B
        dense, lazy = self.nets
        u = torch.tensor(users, dtype=torch.int64, device=DEV)
        items = torch.randint(0, N_TRACKS, (B,), generator=self.gen, device=DEV, dtype=torch.int64).to(torch.int32)
        if self.plan is not None:  # the plan draws its negatives itself: the same draw for the dense run
            nat.check(nat.lib().dcue_sample_inbatch(nat.ptr(self.mts[0]), B, N, nat.ptr(self.neg),
                                                    nat.stream_handle()), "sample")
            neg = self.neg
        else:
            neg = torch.randint(0, B, (B, N), generator=self.gen, device=DEV, dtype=torch.int64).to(torch.int32)
        losses = []
        for net, opt in zip(self.nets, self.opts):
            if net is lazy and self.plan is not None:
                self.plan.step(u, items)
                losses.append(self.plan.loss.detach().clone())
                continue
            _, _, _, loss = net.native_forward(u, self.tracks, items, N, nat.LAYOUT_GATHER, neg, train=True,
                                               margin=0.2)
            losses.append(loss.clone())
            net.native_backward(None)
            opt.step()
        self.t += 1
        self.batches[self.t] = set(users)
        assert torch.equal(losses[0].reshape(()), losses[1].reshape(())), "step %d: loss differs" % self.t
        st = self.opts[0]._adam_state()
        self.dense_hist.append((self.t, dense.user_embd.embeddings.weight.detach().clone(), st["em"].clone(),
                                st["ev"].clone()))

    def steps(self, n):
        for _ in range(n):
            self.step(self.hot())

    def dense_at(self, t):
        for e in self.dense_hist:
            if e[0] == t:
                return tuple(x.double() for x in e[1:])
        raise KeyError(t)

    def touched(self, lo, hi):  # rows in a batch of steps lo < t <= hi
        out = set()
        for t in range(lo + 1, hi + 1):
            out |= self.batches[t]
        return out

    def snap(self):
        """Raw clocks and log header of the deferred optimizer (device copies only)."""
        if self.plan is not None:
            self.plan.sync()
        torch.cuda.synchronize()
        st = self.opts[1]._moments
        clk = st["emb_step"].cpu().numpy().astype(np.int64)
        raw = st["emb_log"][:32].cpu().numpy()
        hdr, fhdr = raw.view(np.int32), raw.view(np.float32)
        assert (clk >= 0).all(), "a row clock left in progress"
        assert hdr[0] == self.t and hdr[4] == CAP
        return Snap(int(hdr[0]), int(hdr[1]), int(hdr[5]), fhdr[6], fhdr[7], (clk & FROZEN) != 0,
                    clk & (FROZEN - 1))

    def flush_and_compare(self, where):
        if self.plan is not None:
            self.plan.sync()
        torch.cuda.synchronize()
        self.opts[1].flush()
        torch.cuda.synchronize()
        _assert_equal_state(_state(self.nets[0], self.opts[0]), _state(self.nets[1], self.opts[1]), where)

    def close(self):
        if self.plan is not None:
            self.plan.close()
            self.plan = None


def _lag_ok(s, where):
    """No frozen row further behind than the refresh allows: its effective clock is max(clock,
    flush_step) -- a full flush brings every row current and leaves the clocks (dcue.h flush_step)."""
    lag = s.T - np.maximum(s.low, s.F)
    assert (lag[s.bit] <= MAX_LAG).all(), "%s: a frozen row is %d steps behind" % (where, lag[s.bit].max())


def _check_freeze(run, s, S, eps, where, most=True):
    """Assertion 1: the rows an independent float64 evaluation of the bound says must be frozen are,
    and no row that breaks the bound by more than the float32 evaluation's slack is."""
    S, eps = float(S), float(eps)
    lim = 2.0 ** -27
    # plans issue a step's slice one step late: every row met a slice within cap + 1 steps
    p, m, v = run.dense_at(s.T - (CAP + 1))
    must = (((m == 0) & (v == 0)) | (4.0 * S * m.abs() <= eps * p.abs() * lim)).all(dim=1).cpu().numpy()
    p, m, v = run.dense_at(s.T)
    must_not = (S * m.abs() > 4.0 * eps * p.abs() * lim).any(dim=1).cpu().numpy()
    moments = ((m != 0) | (v != 0)).any(dim=1).cpu().numpy()
    recent = np.zeros(N_USERS, dtype=bool)
    recent[sorted(run.touched(s.T - (CAP + 1), s.T))] = True
    cold = np.zeros(N_USERS, dtype=bool)
    cold[COLD] = True
    need = must & cold & ~recent
    frozen_cold = s.bit & moments & cold
    print("%s: step %d, %d cold rows frozen with moments, %d must be, %d rows must not be, %d frozen in all"
          % (where, s.T, frozen_cold.sum(), need.sum(), must_not.sum(), s.bit.sum()))
    assert not most or frozen_cold.any(), "%s: no cold row with moments froze" % where
    assert not most or need.sum() * 2 >= len(COLD), "%s: only %d cold rows must be frozen; lengthen the idle phase" % (
        where, need.sum())
    assert s.bit[need].all(), "%s: rows %s meet the bound and are not frozen" % (where, np.nonzero(need & ~s.bit)[0])
    assert not s.bit[must_not].any(), "%s: rows %s break the bound and are frozen" % (
        where, np.nonzero(must_not & s.bit)[0])
    _lag_ok(s, where)
    return int(frozen_cold.sum()), int(need.sum())


def _returns(run, never, where):
    """Phase C: frozen rows come back. Returns the cold rows used."""
    s = run.snap()
    _, m, v = run.dense_at(s.T)
    moments = ((m != 0) | (v != 0)).any(dim=1).cpu().numpy()
    behind = s.bit & moments & (np.maximum(s.low, s.F) < s.T)
    cand = [r for r in COLD if behind[r]]
    assert len(cand) >= 9, "%s: only %d frozen cold rows lag behind" % (where, len(cand))
    picks = [cand[i * (len(cand) - 1) // 8] for i in range(9)]  # spread over the slices' chunks
    assert len(set(picks)) == 9
    f = picks[4]
    eight = picks[:4] + picks[5:]
    h = run.hot()
    for users in (eight, [f, h[0], h[1], f, h[2], h[3], h[4], h[5]], list(never) + h[4:]):
        before = run.snap()
        run.step(users)  # (asserts the loss equal to the dense run's)
        after = run.snap()
        rows = np.array(sorted(set(users)))
        assert (after.low[rows] == after.T).all(), "%s: a returned row's clock is not the step's" % where
        # The step's Adam stores the clock with the bit clear. An eager step then runs its own slice
        # (rows of chunk t mod cap) before anything can be read, and that slice rightly freezes a
        # returned row again when its hinge terms were all inactive (gradient exactly 0: the moments
        # stay as small as they were; about a tenth of the rows here). So: bit clear, except for rows
        # of that chunk which still meet the bound after the step; plans run the slice a step later.
        p, m, v = run.dense_at(after.T)
        breaks = (float(after.S) * m.abs() > 4.0 * float(after.eps) * p.abs() * 2.0 ** -27).any(dim=1).cpu().numpy()
        k = after.T % CAP
        in_slice = (rows >= N_USERS * k // CAP) & (rows < N_USERS * (k + 1) // CAP) & (run.plan is None)
        assert not after.bit[rows][~in_slice | breaks[rows]].any(), \
            "%s: a returned row kept the frozen bit (rows %s)" % (where, rows[after.bit[rows]])
        assert breaks[rows].any(), "%s: no returned row took a gradient" % where
        print("%s: step %d returned rows %s (frozen before: %d, steps behind: up to %d, frozen again by the "
              "step's slice: %d)" % (where, after.T, rows.tolist(), before.bit[rows].sum(),
                                     (before.T - np.maximum(before.low, before.F))[rows].max(),
                                     after.bit[rows].sum()))
    return picks


def _scenario(E, variant, use_plan, betas=(0.6, 0.99), eps=EPS, len_b=LEN_B):
    run = _Run(E, use_plan, betas, eps)
    try:
        _phases(run, variant, betas, eps, len_b)
    finally:
        run.close()


def _phases(run, variant, betas, eps, len_b):
    lazy_opt = run.opts[1]
    g = lazy_opt.param_groups[0]
    # ---- A: one gradient step for each of rows 0..95
    for s in range(LEN_A):
        users = list(range(B * s, B * s + B))
        if s == 1:
            users[1] = users[0]  # a user twice in one batch (row 9 takes its first step in B)
        run.step(users)
    # ---- B: idle
    S0 = np.float32(LR / (1.0 - betas[0]))
    run.steps(len_b * 5 // 8)
    # part of the way: the rows near the bound (no count asked for; the sets are printed)
    _check_freeze(run, run.snap(), S0, np.float32(eps), "B, 5/8 of the way", most=False)
    run.steps(len_b - len_b * 5 // 8)
    sB = run.snap()
    assert sB.start == 1 and sB.S == S0 and sB.eps == np.float32(eps)
    _check_freeze(run, sB, S0, np.float32(eps), "end of B")
    run.flush_and_compare("flush at the end of B")  # frozen rows of any age (k_emb_flush)
    run.steps(LEN_LAG)
    # ---- C: return
    _returns(run, range(96, 100), "C")
    sC = run.snap()
    # ---- D: refresh
    run.steps(LEN_D)
    sD = run.snap()
    _, m, v = run.dense_at(sD.T)
    moments = ((m != 0) | (v != 0)).any(dim=1).cpu().numpy()
    away = np.ones(N_USERS, dtype=bool)
    away[sorted(run.touched(sC.T, sD.T))] = False
    cold = np.zeros(N_USERS, dtype=bool)
    cold[COLD] = True
    refreshed = cold & away & moments & sC.bit & sD.bit & (sD.low > sC.low)
    print("D: steps %d..%d, %d cold frozen rows refreshed (m / v only)" % (sC.T, sD.T, refreshed.sum()))
    assert refreshed.any(), "no frozen row was refreshed in D"
    _lag_ok(sD, "end of D")
    assert (sD.T - sD.low[sD.bit] <= MAX_LAG).all(), "a frozen row's own clock is more than 8 cap + cap behind"
    run.flush_and_compare("flush at the end of D")
    run.steps(LEN_LAG)
    # ---- E: the epoch changes (or a checkpoint round trip)
    sE0 = run.snap()
    t_e = run.t + 1
    n_frozen = int(sE0.bit.sum())
    assert sE0.start == 1 and (sE0.bit & moments & (sE0.low < sE0.T)).any(), "nothing for the thaw to replay"
    if variant == "ckpt":
        sd = lazy_opt.state_dict()
        lazy_opt.load_state_dict(sd)
        s = run.snap()
        assert not s.bit.any() and (s.low == 0).all() and s.start == 0 and s.F == s.T
        _assert_equal_state(_state(run.nets[0], run.opts[0]), _state(run.nets[1], run.opts[1]), "after the reload")
        g = lazy_opt.param_groups[0]  # (load_state_dict rebuilds the groups)
    elif variant == "lr":
        run.group(lr=LR * 20)
    elif variant == "eps":
        run.group(eps=eps / 10)
    elif variant == "betas":
        run.group(betas=(0.7, betas[1]))
    elif variant == "wd":
        run.group(weight_decay=WD_E)
    else:
        raise ValueError(variant)
    run.step(run.hot())
    s = run.snap()
    # thaw: whatever carries the bit now was frozen again by this step's own slice
    assert (s.low[s.bit] >= t_e - 1).all(), "a frozen row survived the epoch's end un-thawed"
    print("E (%s): step %d, %d frozen rows thawed, %d frozen again by the step's slice"
          % (variant, t_e, 0 if variant == "ckpt" else n_frozen, s.bit.sum()))
    t_open = t_e
    if variant == "wd":
        assert s.start == 0 and not s.bit.any()
        for _ in range(LEN_WD - 1):
            run.step(run.hot())
            s = run.snap()
            assert s.start == 0 and not s.bit.any(), "a row froze under weight decay"
        run.group(weight_decay=0.0)
        t_open = run.t + 1
        run.step(run.hot())
        s = run.snap()
    S1 = np.float32(float(g["lr"]) / (1.0 - float(g["betas"][0]) ** t_open))
    eps1 = np.float32(float(g["eps"]))
    assert s.start == t_open and s.S == S1 and s.eps == eps1, (s.start, s.S, s.eps, t_open, S1, eps1)
    # ---- F: re-freeze under the new epoch, then return again
    # B's length plus the decay the 20 x larger S needs, ln 20 / ln(1 / beta1) steps (6 at beta1 = 0.6)
    run.steps(len_b + int(np.ceil(np.log(20.0) / np.log(1.0 / betas[0]))) - 1)
    sF = run.snap()
    assert sF.start == t_open and sF.S == S1 and sF.eps == eps1
    _check_freeze(run, sF, S1, eps1, "end of F")
    _returns(run, range(100, 104), "F")
    # ---- end
    probe = torch.arange(N_USERS, device=DEV)
    run.close()
    for net in run.nets:
        net.eval()
    assert torch.equal(run.nets[0].user_features(probe), run.nets[1].user_features(probe)), \
        "eval-mode user features differ"
    run.flush_and_compare("the end")


@pytest.mark.parametrize("variant", ["lr", "eps", "betas", "wd", "ckpt"])
def test_frozen_rows_eager_float4(variant):
    """E = 40: the float4 paths of the slices and the full flush; every epoch change and the checkpoint."""
    _scenario(40, variant, False)


@pytest.mark.parametrize("E", [30, 300])
def test_frozen_rows_eager_scalar_and_wide(E):
    """E = 30: the scalar (E % 4 != 0) paths, without weight decay so that the epoch exists. E = 300: more
    than one element per thread in k_emb_grad_adam, whole groups of loads in k_user_fwd."""
    _scenario(E, "lr", False)


@pytest.mark.parametrize("E,variant", [(40, "lr"), (40, "wd"), (30, "lr"), (30, "wd")])
def test_frozen_rows_plan(E, variant):
    """TrainPlan.step with the deferred optimizer: k_user_fwd's frozen claim (claimed == 2) and its wait for
    a frozen row listed twice, the slice issued one step late. The dense reference is an eager run fed
    the plan's own negative draws."""
    _scenario(E, variant, True)


def test_frozen_rows_default_beta1():
    """beta1 = 0.9 (the trainer's default) with eps = 1e-4: m decays by 0.9 a step, so the bound asks for
    some 240 idle steps (S = 1e-2, |m| <= 1.9e-11 |p| from 0.1 |g|); the idle phases are 320 steps long."""
    _scenario(40, "lr", False, betas=(0.9, 0.99), eps=1e-4, len_b=320)
