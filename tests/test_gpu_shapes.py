"""The training step and the eval tower against the fp64 oracle at every launch-shape regime.

Every item-tower launch picks its kernel variant on the host from the item count M (row tiles per
workgroup, the DEEP and split-f16 instantiations, split-K depth and chunk length, items per
item-gradient workgroup) and the score kernel from N. tests/launch_shape_cases.py lists shapes that
between them select every variant a step on 2..8,192 items can select (tests/
test_launch_shapes_cpu.py proves the closure on the host); each runs here as a TrainPlan, as
tests/test_gpu_benchshape.py does at the bench shape, against oracle/dcue_oracle.py in fp64 on the
literal [pos; neg] stack:

  launch 1  scores, user / item features, loss and BN running statistics within 1e-4 of the tensor's
            largest value; storage pads zero; the GPU's max-pool argmax and ReLU decisions equal
            fp64's off near-ties (1e-5 of the layer's scale), the near-tie windows -- counted on the
            oracle alone -- at most 0.1 % of a layer's; every dense gradient and the embedding rows
            within 1e-4 of the fp64 oracle run on the GPU's route;
  step      plan.step (launch + fused NativeAdam): loss within 1e-4; catalogue plans repeat the batch
            (the oracle's gradients are already there), in-batch plans draw new negatives;
  launch 2  a new batch: loss within 1e-4 of the oracle's forward with its own Adam-stepped
            parameters, every parameter within 2 lr + 1e-4 max of them.

Data: a 300-track fp16-exact table with repeating item ids, users drawn from 50.

The two largest catalogue shapes, (100, 40) and (128, 63), are the smallest that put the input
gradients of layers 4 and 5 on split-f16 MFMA (M Lin >= 8,192; the report confirms both). The oracle
is most of a case's time: 9.8 s for M = 8,192, the slowest; under 1 s below M = 1,000.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import launch_shape_cases as C
from test_gpu_benchshape import _check_decisions, _close, _gpu_route

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
E, N_USERS, N_TRACKS = 300, 50, 300
LR = 1e-4
TIE = 1e-5
NEAR_TIE_CAP = 1e-3  # share of a layer's windows; the oracle's own share on this input is <= 0.013 %

# Tolerances above the project's 1e-4 bar, as {case id: {tensor: fp32-vs-fp64 spread of the oracle itself}}:
# the test then allows max(1e-4, 8 x spread) for that tensor (the fold-in tests' margin). Never derived
# from the library's output. Needed at M = 2 only: BatchNorm over two items maps every channel with one
# position to +-1 whatever the input, so the gradient below BN5 / BN4 is what is left of an exact
# cancellation -- of the order of eps / var -- and fp32 itself (the oracle run in fp32 on the CPU
# against itself in fp64, unrouted, the batch of launch 1) is no closer than this:
_L14 = ["conv.bn0.weight", "conv.bn0.bias"] + ["conv.%s%d.%s" % (m, l, t) for l in (1, 2, 3, 4)
                                               for m in ("layer", "bn") for t in ("weight", "bias")][:-2]


def _spreads(values, tail=()):
    d = {"grad " + k: v for k, v in zip(_L14, values)}
    d.update({"grad " + k: v for k, v in tail})
    return d


SPREAD = {
    "catalogue-bn-B1-N1-d32-H32": _spreads(
        [1.58e-4, 1.47e-4, 1.47e-4, 1.67e-4, 1.87e-4, 1.88e-4, 1.42e-4, 2.18e-4, 1.72e-4, 1.46e-4, 1.38e-4, 2.03e-4,
         1.35e-4, 1.30e-4, 1.52e-4, 1.08e-4]),
    "inbatch-bn-B2-N1-d32-H32": _spreads(
        [2.29e-2, 7.52e-2, 2.66e-2, 5.32e-2, 1.81e-2, 3.33e-2, 1.68e-2, 4.69e-2, 1.05e-2, 2.64e-2, 8.94e-3, 5.00e-2,
         2.47e-3, 9.46e-3, 2.58e-3, 2.12e-3],
        [("conv.bn4.weight", 2.01e-5), ("conv.bn4.bias", 2.76e-5), ("conv.layer5.weight", 2.21e-5),
         ("conv.layer5.bias", 1.34e-5)]),
    "catalogue-bn-B1-N1-d128-H128": _spreads(
        [1.99e-4, 2.02e-4, 2.00e-4, 2.01e-4, 2.02e-4, 2.00e-4, 2.00e-4, 2.01e-4, 2.01e-4, 2.01e-4, 1.97e-4, 2.02e-4,
         2.01e-4, 2.02e-4, 2.01e-4, 3.59e-2],
        [("conv.bn4.weight", 2.84e-4), ("conv.bn4.bias", 2.73e-4), ("conv.layer5.weight", 3.15e-4),
         ("conv.layer5.bias", 3.14e-4), ("conv.bn5.weight", 1.29e-5), ("conv.bn5.bias", 3.59e-5),
         ("conv.fc.weight", 1.61e-5)]),
}

_DATA = {}


def _tracks_cpu():
    """The shared track table: X [300, 128, 131] fp32 holding fp16 values."""
    if "X" not in _DATA:
        gen = torch.Generator().manual_seed(5)
        _DATA["X"] = torch.randn(N_TRACKS, 128, 131, generator=gen).half().float()
    return _DATA["X"]


def _tracks():
    """The track table and its device rows [n][131][128] fp16."""
    X = _tracks_cpu()
    if "table" not in _DATA:
        _DATA["table"] = X.half().transpose(1, 2).contiguous().to(DEV)
    return X, _DATA["table"]


def _near_tie_share(pre, tie=TIE):
    """Share of each layer's pool windows whose ReLU or argmax decision is a near-tie in the fp64
    oracle (what _check_decisions leaves out)."""
    from oracle import dcue_oracle as O
    share = {}
    for l, (k, pad, pool) in enumerate(O.CONV_SPECS, start=1):
        c = pre[l - 1]
        scale = float(c.abs().max())
        Lp = c.shape[2] // pool
        w = c[:, :, :Lp * pool].reshape(c.shape[0], c.shape[1], Lp, pool)
        top = w.topk(min(2, pool), dim=3).values
        near = top[..., 0].abs() <= tie * scale
        if pool > 1:
            near |= (top[..., 0] > 0) & (top[..., 0] - top[..., 1] <= tie * scale)
        share[l] = float(near.double().mean())
    return share


def oracle_params(case):
    """The case's parameters as the oracle holds them (fp64) -- DCUENet's own under the same seed."""
    from oracle import dcue_oracle as O
    _, model_type, _, _, D, H = case
    torch.manual_seed(0)
    p, b = O.init_params(D, H, E, N_USERS, model_type)
    return ({k: v.double() for k, v in p.items()},
            {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()})


class Batches:
    """A case's batches, drawn on the CPU alone: users from 50, items from the 300 tracks, in-batch
    negatives from numpy's sampler (the plan's MT19937 stream under the same seed)."""
    SEED = 17

    def __init__(self, case):
        self.layout, _, self.B, self.N, _, _ = case
        self.inbatch = self.layout == "inbatch"
        self.gen = torch.Generator().manual_seed(7 + C.case_items(case))
        self.rs = np.random.RandomState(self.SEED)
        self.X = _tracks_cpu()

    def draw(self, r=None):
        """(u, pos_items, neg_items, r): r the in-batch draws (given: kept, only the items redrawn)."""
        from oracle import dcue_oracle as O
        B, N = self.B, self.N
        u = torch.randint(0, N_USERS, (B,), generator=self.gen)
        pos_items = torch.randint(0, N_TRACKS, (B,), generator=self.gen)
        if self.inbatch:
            if r is None:
                r = torch.from_numpy(O.inbatch_negatives(self.rs, B, N))
            return u, pos_items, pos_items[r.reshape(-1)].reshape(B, N), r
        return u, pos_items, torch.randint(0, N_TRACKS, (B, N), generator=self.gen), None

    def literal(self, pos_items, neg_items):
        """The reference's [pos; neg] inputs in fp64."""
        return self.X[pos_items].double(), self.X[neg_items.reshape(-1)].reshape(self.B, self.N, 128, 131).double()

    def first(self, p, b):
        """The batch of launch 1 with its fp64 pre-pool conv outputs and near-tie shares. A batch whose
        near-tie share -- a property of the oracle and the data alone -- is above the cap is drawn
        again (a layer of a 3-item batch has under 1,000 windows: one near-tie is over 0.1 %)."""
        from oracle import dcue_oracle as O
        r = None
        for _ in range(8):
            u, pos_items, neg_items, r = self.draw(r)
            pos, neg = self.literal(pos_items, neg_items)
            pre = O.conv_trace(p, b, torch.cat([pos, neg.reshape(self.B * self.N, 128, 131)]))
            share = _near_tie_share(pre)
            if max(share.values()) <= NEAR_TIE_CAP:
                break
        return u, pos_items, neg_items, r, pos, neg, pre, share


class _Checks:
    """Collects every comparison of a case, prints each figure, and fails once at the end with all of
    them -- one run shows everything a case misses."""

    def __init__(self, cid):
        self.cid, self.bad, self.spread = cid, [], SPREAD.get(cid, {})

    def close(self, got, ref, what, key=None):
        got = torch.as_tensor(got).double().cpu()
        ref = torch.as_tensor(ref).double().cpu().reshape(got.shape)
        tol = max(1e-4, 8 * self.spread.get(key or what, 0.0))
        mx = max(float(ref.abs().max()), 1e-30)
        print("  %-46s err %.3e of max %.3e (%.2e, tol %.1e)" % (what, float((got - ref).abs().max()), mx,
                                                               float((got - ref).abs().max()) / mx, tol))
        try:
            _close(got, ref, tol, tol, what)
        except AssertionError as e:
            self.bad.append(str(e))

    def that(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def done(self):
        assert not self.bad, "%s: %d checks failed:\n  %s" % (self.cid, len(self.bad), "\n  ".join(self.bad))


def run_case(case):
    from dcrecommend import _native as nat
    from dcrecommend.dcue.dcue import DCUENet
    from dcrecommend.dcue.plan import TrainPlan
    from dcrecommend.optim import NativeAdam
    from oracle import dcue_oracle as O
    from test_gpu_parity import assert_storage_pads_zero
    layout, model_type, B, N, D, H = case
    inbatch = layout == "inbatch"
    M = C.case_items(case)
    cid = C.case_id(case)
    print("%s: M = %d, variants %s" % (cid, M, sorted(C.keys_of(C.shape_of(nat, case)), key=str)))
    ck = _Checks(cid)
    X, table = _tracks()
    torch.manual_seed(0)
    net = DCUENet({"feature_dim": D, "conv_hidden": H, "user_embdim": E, "user_count": N_USERS,
                   "model_type": model_type}).to(DEV).train()
    p, b = oracle_params(case)
    adam = O.AdamState(p)
    opt = NativeAdam(net.parameters(), LR, (0.9, 0.99), 1e-8, 0, defer_embedding=True, flush_every=64)
    bt = Batches(case)
    mt = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=DEV)
    nat.check(nat.lib().dcue_mt_seed(nat.ptr(mt), bt.SEED, nat.stream_handle()), "mt_seed")
    plan = TrainPlan(net, table, B, N, mt_state=mt if inbatch else None, optimizer=opt)
    dims = net._flat["dims"]
    off = nat.workspace_outputs(dims, B, N, M)
    Ds = nat.storage_dims(dims).feature_dim

    def ws_view(o, n, shape):
        return net._ws[o:o + 4 * n].view(torch.float32).view(shape)

    def loss_gpu():
        return ws_view(off[3], 1, ())

    def on_gpu(u, pos_items, neg_items):
        items = pos_items if inbatch else torch.cat([pos_items, neg_items.reshape(-1)])
        return u.to(DEV), items.to(torch.int32).to(DEV)

    # ---- launch 1: forward, decisions, gradients
    u, pos_items, neg_items, r, pos, neg, pre, share = bt.first(p, b)
    plan.launch(*on_gpu(u, pos_items, neg_items))
    torch.cuda.synchronize()
    if inbatch:
        ck.that(torch.equal(plan.neg_item.cpu().long(), r), "in-batch draws differ from numpy")
    b_run = {k: v.clone() for k, v in b.items()}
    with torch.no_grad():
        rs_, ruf, rpf, rnf = O.forward(p, b_run, u, pos, neg, train=True)
        ref_loss = O.hinge_loss(rs_)
    ck.that(float(ref_loss) > 0, "the oracle's loss is 0: the case has no gradient to check")
    ck.close(ws_view(off[0], B * N, (B, N)), rs_, "scores")
    uf_s = ws_view(off[1], B * Ds, (B, Ds)).cpu()
    ck.close(uf_s[:, :D], ruf, "user feats")
    feats_s = ws_view(off[2], M * Ds, (M, Ds)).cpu()
    ck.that(not bool(uf_s[:, D:].any()) and not bool(feats_s[:, D:].any()), "feature storage pads not zero")
    ck.close(feats_s[:B, :D], rpf, "positive feats")  # (item_tower squeezes: reshaped to the GPU's)
    if not inbatch:
        ck.close(feats_s[B:, :D].reshape(B, N, D), rnf, "negative feats")
    ck.close(loss_gpu(), ref_loss, "loss")
    for k, v in net.state_dict().items():  # BN running statistics after one train forward
        if "running" in k:
            ck.close(v, b_run[k], k)
    rows = torch.cat([torch.arange(B), r.reshape(-1)]) if inbatch else torch.arange(M)
    route = _gpu_route(net, nat, B, N, M, rows, D, H)
    print("  near-tie share per layer (fp64 oracle): %s" % {l: "%.4f%%" % (100 * s) for l, s in share.items()})
    ck.that(max(share.values()) <= NEAR_TIE_CAP, "near-tie windows above 0.1 %% of a layer's: %s" % share)
    try:
        flips = _check_decisions(pre, route, TIE)
    except AssertionError as e:
        flips = None
        ck.bad.append(str(e))
    del pre
    b_grad = {k: v.clone() for k, v in b.items()}
    _, g64, _ = O.loss_and_grads(p, b_grad, u, pos, neg, route=route)
    ck.that(float(g64["conv.layer1.weight"].abs().max()) > 0, "the oracle's conv-1 gradient is all zero")
    named = dict(net.named_parameters())
    for k, g_ref in g64.items():
        got = net.embedding_grad_dense() if k == "user_embd.embeddings.weight" else named[k].grad
        ck.close(got, g_ref, "grad %s" % k)
    print("  near-tie windows decided differently: %s" % flips)
    try:
        assert_storage_pads_zero(net)
    except AssertionError as e:
        ck.bad.append(str(e))

    # ---- one fused step (launch + Adam)
    if inbatch:  # new negatives are drawn whatever the batch: a new batch, the oracle's own decisions
        u, pos_items, neg_items, r = bt.draw()
        plan.step(*on_gpu(u, pos_items, neg_items))
        torch.cuda.synchronize()
        pos, neg = bt.literal(pos_items, neg_items)
        ck.that(torch.equal(plan.neg_item.cpu().long(), r), "step: in-batch draws differ from numpy")
        ref_loss, g64, _ = O.loss_and_grads(p, b_grad, u, pos, neg)
    else:        # the same batch: the same forward and gradients, checked above
        plan.step(*on_gpu(u, pos_items, neg_items))
        torch.cuda.synchronize()
    ck.close(loss_gpu(), ref_loss, "step loss")
    adam.step(p, g64, LR)
    del g64, pos, neg

    # ---- launch 2: the stepped parameters on a new batch
    u, pos_items, neg_items, r = bt.draw()
    plan.launch(*on_gpu(u, pos_items, neg_items))
    torch.cuda.synchronize()
    pos, neg = bt.literal(pos_items, neg_items)
    if inbatch:
        ck.that(torch.equal(plan.neg_item.cpu().long(), r), "launch 2: in-batch draws differ from numpy")
    with torch.no_grad():
        ref_loss = O.hinge_loss(O.forward(p, b_grad, u, pos, neg, train=True)[0])
    ck.close(loss_gpu(), ref_loss, "loss after the step")
    opt.flush()
    torch.cuda.synchronize()
    sd = net.state_dict()
    worst = 0.0
    for k, ref in p.items():
        diff = float((sd[k].detach().double().cpu() - ref).abs().max())
        tol = 2 * LR + 1e-4 * float(ref.abs().max())
        worst = max(worst, diff / tol)
        ck.that(diff <= tol, "%s after the step: %.3e off (allowed %.3e)" % (k, diff, tol))
    print("  parameters after the step: worst %.2f of 2 lr + 1e-4 max" % worst)
    plan.close()
    ck.done()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_step_against_oracle(case):
    run_case(case)


# ------------------------------------------------------------------------------------ eval tower
EVAL_M = (1, 2, 17, 129, 497, 2049, 8191)


@pytest.mark.parametrize("H,d", [(32, 32), (128, 128)])
def test_eval_tower_against_oracle(H, d):
    """dcue_item_tower_eval, as DCUE._factors_over calls it (chunks of up to 8,192 items with a ragged
    last one), against O.item_tower(train=False) in fp64: random gamma, beta and running statistics,
    so eval BatchNorm is not the identity. H = d = 128 up to M = 497."""
    from dcrecommend import _native as nat
    from dcrecommend.dcue.dcue import DCUENet
    from oracle import dcue_oracle as O
    X, table = _tracks()
    torch.manual_seed(0)
    net = DCUENet({"feature_dim": d, "conv_hidden": H, "user_embdim": E, "user_count": N_USERS,
                   "model_type": C.BN}).to(DEV)
    torch.manual_seed(0)
    p, b = O.init_params(d, H, E, N_USERS, C.BN)
    gen = torch.Generator().manual_seed(11)
    for k in p:
        if ".bn" in k:
            p[k] = (0.5 + torch.rand(p[k].shape, generator=gen)) if k.endswith("weight") else \
                0.3 * torch.randn(p[k].shape, generator=gen)
    for k in b:
        if k.endswith("running_mean"):
            b[k] = 0.3 * torch.randn(b[k].shape, generator=gen)
        elif k.endswith("running_var"):
            b[k] = 0.5 + torch.rand(b[k].shape, generator=gen)
    net.load_state_dict({**p, **b})
    net.eval()
    net._require_device()
    p64 = {k: v.double() for k, v in p.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}
    X64 = X.double()
    tr = net._tracks(table)
    bad = []
    for M in EVAL_M:
        if H == 128 and M > 497:
            continue
        items = torch.randint(0, N_TRACKS, (M,), generator=gen)
        it = items.to(torch.int32).to(DEV)
        out = torch.full((M, net._ds), float("nan"), device=DEV)
        ws = net._workspace(1, 0, M)
        nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(net._model_struct()), ctypes.byref(tr), nat.ptr(it),
                                                 M, nat.ptr(ws), ws.numel(), nat.ptr(out), nat.stream_handle()),
                  "dcue_item_tower_eval")
        torch.cuda.synchronize()
        with torch.no_grad():
            ref = O.item_tower(p64, b64, X64[items], train=False).reshape(M, d)  # (squeezed at M = 1)
        got = out.cpu()
        err = float((got[:, :d].double() - ref).abs().max()) / float(ref.abs().max())
        print("eval tower H=%d M=%d: err %.3e of max" % (H, M, err))
        try:
            assert not bool(got[:, d:].any()), "storage pads not zero"
            _close(got[:, :d], ref, 1e-4, 1e-4, "eval features at M = %d" % M)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# -------------------------------------------------------------------------------- forced tilings
FORCED_CASES = [c for c in C.CASES if c[:4] in (("catalogue", C.BN, 5, 12), ("catalogue", C.BN, 43, 2)) and c[5] == 32]


def test_forced_tilings_against_oracle():
    """DCUE_ROWS_TW (read once per process) forces 1, 2, 3, 4 or 8 row tiles per workgroup wherever
    the slab fits: one worker process per value runs the (5, 12) and (43, 2) catalogue cases with
    the same checks, reaching tile / ragged-edge combinations the planner does not pick today. One
    after another, each with a time limit, stopping at the first that fails."""
    assert len(FORCED_CASES) == 2
    for tw in (1, 2, 3, 4, 8):
        env = dict(os.environ, DCUE_ROWS_TW=str(tw))
        p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "shapes_worker.py")], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        print(p.stdout[-6000:])
        assert p.returncode == 0, "DCUE_ROWS_TW=%d failed:\n%s" % (tw, p.stdout[-6000:])
        assert "forced tilings ok: TW %d" % tw in p.stdout
