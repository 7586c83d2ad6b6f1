"""The text conv and its weight gradient against the fp64 oracle, per kernel, at every launch regime.

launch_text_fwd picks its kernel (the gather-once k_text_fwd_full or the chunked k_text_fwd), the
position tiles, waves, weight-prefetch depth, compile-time chunk count and XCD spread on the host from
M, T, word_dim and text_dim; launch_text_wgrad picks the item chunks. tests/text_shape_cases.py lists
shapes that between them select every variant (tests/test_text_shapes_cpu.py proves the closure on
the host); each runs here as a TrainPlan at d = H = 32 over the 300-track table of
tests/test_gpu_shapes.py, and the text kernels are observed at their own outputs (dcue_workspace_text):

  a  the text features xfc[:, :text_dim] within 1e-4 of max |s| of fp64 text_features;
  b  the argmax bytes tidx equal to the oracle's decision -- the FIRST maximum over the non-PAD
     positions, 255 where it is <= 0 -- off near-ties (top-two gap or |top| within 1e-5 of max |z|; an
     exact tie is no near-tie), near-ties, counted on the oracle alone, at most 0.1 % of the (item,
     channel) pairs; storage channels >= text_dim all 255;
  c  k_text_wgrad / k_text_wreduce alone: dW[o][c][k] = sum_i g[i][o] words[tok[i][t* + k - 1]][c] and
     db formed in fp64 on the host from the dtp and tidx the GPU left, per element within
     2 (n_live + nchunk) 2^-24 sum_i |g x| -- the running-sum bound of the kernel's in-order fp32 FMA
     chain plus the chunk adds, doubled; exactly 0 where the sum is empty;
  d  end to end: scores, loss and the gradients of text.conv.{weight, bias} and conv.fc.{weight, bias}
     within 1e-4 of the tensor's max of TO.loss_and_grads in fp64 run on the GPU's routes (the audio
     layers' and tidx); storage pads zero;
  e  one plan.step: loss within 1e-4, the text conv parameters within 2 lr + 1e-4 max of the oracle's
     Adam step.

Then the eval tower at M = 1 and 130, sentence content (all-PAD, BOS + EOS only, full-length, PAD
inside and on the left, maxima at t = 0 and t = T - 1), the first-maximum rule on exact ties (also
with the positions split over two workgroups, DCUE_TEXT_PARTS=2) and word tables scaled by 2^-12,
2^12 and with one row 2^12 times the others.
"""
import os
import subprocess
import sys

import pytest
import torch

import text_shape_cases as C
from test_gpu_benchshape import _gpu_route
from test_gpu_shapes import DEV, E, LR, N_TRACKS, N_USERS, Batches, _tracks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = H = 32
PAD = C.PAD
TIE = 1e-5
NEAR_TIE_CAP = 1e-3
ROW18 = ("catalogue", 3, 5, 17, 100, 64, 60)  # the 18-item row: the widths of the content and range tests

# Tolerances above 1e-4, as {case id: {tensor: fp32-vs-fp64 spread of the oracle itself on the CPU}}: the
# test then allows max(1e-4, 8 x spread) (tests/test_gpu_shapes.py's rule). Never taken from the
# library's output. One is needed: the three items of this batch score 0.0037 and -0.0027 -- differences
# of cosines near 1 -- so a few ulp of a cosine is 1e-4 of the largest score; the oracle itself in fp32
# (unrouted, the batch of launch 1, on the CPU) is 1.49e-5 of that maximum away from its fp64 run. The
# GPU was 1.03e-4 away (3.9e-7 absolute).
SPREAD = {"catalogue-B1-N2-T64-td128-wd292": {"scores": 1.49e-5}}


class _Checks:
    """Collects every comparison of a case, prints each figure, and fails once at the end with all of
    them."""

    def __init__(self, cid):
        self.cid, self.bad, self.spread = cid, [], SPREAD.get(cid, {})

    def within(self, got, ref, what, per_row=False):
        """max |got - ref| <= tol x max |ref| (per_row: row by row, each against its own max)."""
        got = torch.as_tensor(got).double().cpu()
        ref = torch.as_tensor(ref).double().cpu().reshape(got.shape)
        tol = max(1e-4, 8 * self.spread.get(what, 0.0))
        err = (got - ref).abs()
        if per_row:
            mx = ref.abs().flatten(1).max(dim=1).values
            e = err.flatten(1).max(dim=1).values
            rel = float((e / mx.clamp(min=1e-300)).max())
            ok = bool((e <= tol * mx).all())
            print("  %-40s worst row err %.3e of its max (rows' max %.3e .. %.3e)" % (what, rel, float(mx.min()),
                                                                                     float(mx.max())))
        else:
            mx = float(ref.abs().max())
            rel = float(err.max()) / max(mx, 1e-300)
            ok = float(err.max()) <= tol * mx
            print("  %-40s err %.3e of max %.3e (%.2e, tol %.1e)" % (what, float(err.max()), mx, rel, tol))
        if not ok or not bool(torch.isfinite(got).all()):
            self.bad.append("%s: err %.3e of max, allowed %.1e" % (what, rel, tol))
        return rel

    def that(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def done(self):
        assert not self.bad, "%s: %d checks failed:\n  %s" % (self.cid, len(self.bad), "\n  ".join(self.bad))


def first_max(zm):
    """(value, first position) of the maximum over the last axis, -inf rows: position 0."""
    top = zm.max(dim=2).values
    T = zm.shape[2]
    pos = torch.arange(T).expand_as(zm)
    return top, torch.where(zm == top.unsqueeze(2), pos, torch.full_like(pos, T)).min(dim=2).values.clamp(max=T - 1)


def oracle_decisions(p64, tok, tie=TIE, per_item=False):
    """The oracle's text_route [M, text_dim] by the first-maximum rule and the near-tie mask: top-two
    gap (between distinct values: an exact tie is decided by position) or |top| within tie x max |z|.

    per_item (a word table whose rows differ in magnitude by 2^12): max |z| of the case, or of the
    item, is set by the large word, and under tie x that most decisions between ordinary positions
    would count as near-ties (8.6 % of the pairs by the case's max, 0.8 % by the item's: measured on
    the oracle alone, both above the 0.1 % cap). The window there is tie x A, A[i][o][t] = |b[o]| +
    sum_k,c |w[o][c][k]| |x[i][t + k - 1][c]| of the two positions compared -- the quantity the
    rounding error of z[i][o][t] scales with. A <= the case's window wherever the large word is not in
    reach, so it holds more decisions firm than the plain rule does, never fewer of those."""
    from oracle import text_oracle as TO
    with torch.no_grad():
        z = TO.text_preact(p64, tok)
    valid = (tok != PAD).unsqueeze(1)
    zm = z.masked_fill(~valid, float("-inf"))
    some = valid.expand_as(z)
    scale = float(z[some].abs().max()) if bool(some.any()) else 1.0
    top, pos = first_max(zm)
    rest = zm.masked_fill(zm == top.unsqueeze(2), float("-inf")).max(dim=2)
    below = rest.values
    live = torch.isfinite(top)
    if per_item:
        with torch.no_grad():
            A = TO.text_preact({k: v.abs() for k, v in p64.items()}, tok)
        a1 = A.gather(2, pos.unsqueeze(2)).squeeze(2)
        a2 = torch.maximum(a1, A.gather(2, rest.indices.unsqueeze(2)).squeeze(2))
        near = live & ((top.abs() <= tie * a1) | (top - below <= tie * a2))
    else:
        near = live & ((top.abs() <= tie * scale) | (top - below <= tie * scale))
    dec = torch.where(top > 0, pos, torch.full_like(pos, 255))
    return dec, near, zm


def host_text_wgrad(g, route, tok, words64, T):
    """dW [C, E, 3], db [C], their absolute-value sums and the live items per channel, in fp64: g
    [M, C] = dL/ds, route [M, C] the positions (255: none), tok [M, T]."""
    M, Cc = route.shape
    Ew = words64.shape[1]
    dW, S = torch.zeros(Cc, Ew, 3, dtype=torch.float64), torch.zeros(Cc, Ew, 3, dtype=torch.float64)
    db, Sb = torch.zeros(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    nlive = torch.zeros(Cc, dtype=torch.long)
    step = max(1, 4000000 // (Cc * Ew))
    tok = tok.long()
    for i0 in range(0, M, step):
        tt = route[i0:i0 + step]
        live = tt != 255
        gg = torch.where(live, g[i0:i0 + step].double(), torch.zeros((), dtype=torch.float64))
        for k in range(3):
            pos = tt + k - 1
            ok = live & (pos >= 0) & (pos < T)
            X = words64[tok[i0:i0 + step].gather(1, pos.clamp(0, T - 1))] * ok.unsqueeze(2)   # [m, C, E]
            dW[:, :, k] += torch.einsum("io,ioc->oc", gg, X)
            S[:, :, k] += torch.einsum("io,ioc->oc", gg.abs(), X.abs())
        db += gg.sum(0)
        Sb += gg.abs().sum(0)
        nlive += live.sum(0)
    return dW, db, S, Sb, nlive


def check_wgrad(ck, named, g, route, tok, words64, T, td, nchunk, what):
    """Check c on the reference's corner of the gradients."""
    dW, db, S, Sb, nlive = host_text_wgrad(g[:, :td], route[:, :td], tok, words64, T)
    n = (nlive + nchunk).double() * 2.0 * 2.0 ** -24
    worst = 0.0
    for name, got, ref, bound in (("weight", named["text.conv.weight"].grad, dW, n[:, None, None] * S),
                                  ("bias", named["text.conv.bias"].grad, db, n * Sb)):
        got = got.detach().double().cpu()
        err = (got - ref).abs()
        ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
        some = bound > 0
        rel = float((err[some] / bound[some]).max()) if bool(some.any()) else 0.0
        worst = max(worst, rel)
        print("  %-40s worst err %.3f of its bound (max |ref| %.3e, live items <= %d, %d chunks)"
              % ("%s d%s" % (what, name), rel, float(ref.abs().max()), int(nlive.max()), nchunk))
        ck.that(ok, "%s d%s: %d elements beyond 2 (n + nchunk) 2^-24 sum |g x| (worst %.3f of the bound, %d non-zero "
                "where the sum is empty)" % (what, name, int((err > bound).sum()), rel, int(((got != 0) & ~some).sum())))
    return worst


def build(case, words=None, edit=None):
    """(net on the GPU in train mode, oracle p, b in fp64, token table [300, T] on the CPU)."""
    from dcrecommend.dcue.dcue import DCUENet
    from oracle import text_oracle as TO
    layout, B, N, T, td, wd, V = case
    args = {"feature_dim": D, "conv_hidden": H, "user_embdim": E, "user_count": N_USERS, "model_type": C.TEXT,
            "text_dim": td, "word_dim": wd, "text_len": T, "n_words": V, "pad_idx": PAD}
    torch.manual_seed(0)
    net = DCUENet(args)
    torch.manual_seed(0)
    p, b = TO.init_params(D, H, E, N_USERS, td, wd, V)
    if words is not None:
        p["text.embeddings.weight"] = words(p["text.embeddings.weight"])
    if edit is not None:
        edit(p)
    with torch.no_grad():
        for k in ("text.embeddings.weight", "text.conv.weight"):
            dict(net.named_parameters())[k].copy_(p[k])
    gen = torch.Generator().manual_seed(100 + T)
    toks = TO.sentences(gen, N_TRACKS, T, V, PAD, min_len=0 if T == 2 else 1)
    p64 = {k: v.double() for k, v in p.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}
    return net.to(DEV).train(), p64, b64, toks


def first_batch(bt, toks, p, pick=None, per_item=False, tries=8):
    """The batch of launch 1: one whose near-tie share -- the oracle's and the data's alone -- is
    inside the cap (120 pairs at M = 3: a single near-tie would be over 0.1 %)."""
    r = None
    for _ in range(tries):
        u, pos_items, neg_items, r = bt.draw(r)
        if pick is not None:
            pos_items, neg_items = pick
        items = pos_items if bt.inbatch else torch.cat([pos_items, neg_items.reshape(-1)])
        tok = toks[items]
        dec, near, zm = oracle_decisions(p, tok, per_item=per_item)
        share = float(near.double().mean())
        if share <= NEAR_TIE_CAP or pick is not None:
            break
    return u, pos_items, neg_items, r, tok, dec, near, zm, share


def run_case(case, cid=None, toks=None, pick=None, words=None, edit=None, checks="abcde", per_item=False,
             oracle_route=False, expect=None, tries=8):
    """One case under checks a-e. toks: the token table [300, T] (default: BOS + words + EOS + PAD);
    pick: (pos_items [B], neg_items [B, N]) of launch 1 (default: drawn); words / edit: changes to the
    word table / the oracle's parameters before the model takes them; per_item: check a row by row,
    each against its own max |s|, and check b's near-tie window position by position
    (oracle_decisions); tries:
    batches drawn until one is inside the near-tie cap;
    oracle_route: check c also on the oracle's own route (off near-ties); expect(dec, near, zm, tok):
    further assertions on the oracle's decisions. Returns the measured figures."""
    from dcrecommend import _native as nat
    from dcrecommend.dcue.plan import TrainPlan
    from dcrecommend.optim import NativeAdam
    from oracle import dcue_oracle as O
    from oracle import text_oracle as TO
    from test_gpu_parity import assert_storage_pads_zero
    layout, B, N, T, td, wd, V = case
    inbatch = layout == "inbatch"
    M = C.case_items(case)
    cid = cid or C.case_id(case)
    ck = _Checks(cid)
    fig = {}
    net, p, b, toks0 = build(case, words, edit)
    toks = toks0 if toks is None else toks
    print("%s: M = %d, forward %s, weight gradient %s" % (cid, M, C.fwd_key(C.shape_words(nat, case))[1:],
                                                           C.wgrad_key(C.shape_words(nat, case))[1:]))
    X, table = _tracks()
    tok_d = toks.to(DEV)
    opt = NativeAdam(net.parameters(), LR, (0.9, 0.99), 1e-8, 0, defer_embedding=True, flush_every=64)
    bt = Batches((layout, C.TEXT, B, N, D, H))
    mt = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=DEV)
    nat.check(nat.lib().dcue_mt_seed(nat.ptr(mt), bt.SEED, nat.stream_handle()), "mt_seed")
    plan = TrainPlan(net, table, B, N, mt_state=mt if inbatch else None, optimizer=opt, tokens=tok_d)
    dims = net._flat["dims"]
    shape = nat.text_shape(dims, M)
    off = nat.workspace_outputs(dims, B, N, M)
    toff = nat.workspace_text(dims, B, N, M)
    Ds, Cs = nat.storage_dims(dims).feature_dim, nat.text_storage(td)

    def ws_view(o, n, shape_):
        return net._ws[o:o + 4 * n].view(torch.float32).view(shape_)

    def on_gpu(u, pos_items, neg_items):
        items = pos_items if inbatch else torch.cat([pos_items, neg_items.reshape(-1)])
        return u.to(DEV), items.to(torch.int32).to(DEV)

    u, pos_items, neg_items, r, tok, dec, near, zm, share = first_batch(bt, toks, p, pick, per_item, tries)
    print("  near-tie share (fp64 oracle): %.4f%% of %d pairs" % (100 * share, near.numel()))
    ck.that(share <= NEAR_TIE_CAP, "near-ties above 0.1 %% of the (item, channel) pairs: %.3e" % share)
    if expect is not None:
        expect(dec, near, zm, tok)
    plan.launch(*on_gpu(u, pos_items, neg_items))
    torch.cuda.synchronize()
    if inbatch:
        ck.that(torch.equal(plan.neg_item.cpu().long(), r), "in-batch draws differ from numpy")
    xfc = ws_view(toff[0], M * (td + Ds), (M, td + Ds)).cpu()
    dtp = ws_view(toff[1], M * Cs, (M, Cs)).cpu()
    tidx = net._ws[toff[2]:toff[2] + M * Cs].view(M, Cs).cpu().long()
    named = dict(net.named_parameters())
    allpad = (tok == PAD).all(dim=1)
    if bool(allpad.any()):  # a row without a valid position: exactly zero features, no gradient
        ck.that(not bool(xfc[allpad, :td].any()), "an all-PAD row's text features are not exactly 0")
        ck.that(bool((tidx[allpad] == 255).all()), "an all-PAD row's argmax bytes are not all 255")
    ck.that(bool(torch.isfinite(xfc).all()) and bool(torch.isfinite(dtp).all()), "xfc or dtp is not finite")
    # ---- a: the text features
    if "a" in checks:
        with torch.no_grad():
            s64 = TO.text_features(p, tok, PAD)
        ck.that(float(s64.abs().max()) > 0, "the oracle's text features are all zero")
        fig["a"] = ck.within(xfc[:, :td], s64, "text features s", per_row=per_item)
    # ---- b: the argmax bytes
    if "b" in checks:
        got = tidx[:, :td]
        firm = ~near
        wrong = int((got != dec)[firm].sum())
        print("  argmax bytes: %d of %d firm decisions differ, %d near-ties decided differently, %d exact ties"
              % (wrong, int(firm.sum()), int((got != dec)[near].sum()),
                 int(((zm == zm.max(dim=2, keepdim=True).values) & torch.isfinite(zm)).sum(dim=2).gt(1).sum())))
        ck.that(wrong == 0, "tidx differs from the oracle's first maximum at %d firm (item, channel) pairs" % wrong)
        ck.that(bool((tidx[:, td:] == 255).all()), "tidx of the storage channels >= text_dim is not all 255")
        ck.that(bool(((got == 255) | (got < T)).all()), "tidx holds a position >= T")
    # ---- c: the weight gradient from the GPU's own dtp and tidx
    words64 = p["text.embeddings.weight"]
    nchunk = shape["wgrad"]["nchunk"]
    if "c" in checks:
        ck.that(bool((tidx[:, :td] != 255).any()) and float(dtp.abs().max()) > 0, "no text gradient to check")
        fig["c"] = check_wgrad(ck, named, dtp, tidx, tok, words64, T, td, nchunk, "wgrad (GPU route)")
        if oracle_route:  # the oracle's decisions off near-ties: a tie decided for a later position shows here
            fig["c_oracle"] = check_wgrad(ck, named, dtp, torch.where(near, tidx[:, :td], dec), tok, words64, T, td,
                                          nchunk, "wgrad (oracle route)")
    # ---- d: end to end on the GPU's routes
    g64 = None
    if "d" in checks:
        rows = torch.cat([torch.arange(B), r.reshape(-1)]) if inbatch else torch.arange(M)
        route = _gpu_route(net, nat, B, N, M, rows, D, H)
        pos, neg = bt.literal(pos_items, neg_items)
        pt, nt = toks[pos_items], toks[neg_items.reshape(-1)].reshape(B, N, T)
        ref_loss, g64, (rs_, _, _, _) = TO.loss_and_grads(p, {k: v.clone() for k, v in b.items()}, u, pos, neg, pt, nt,
                                                          PAD, route=route, text_route=tidx[rows, :td])
        ck.that(float(ref_loss) > 0, "the oracle's loss is 0: the case has no gradient to check")
        fig["scores"] = ck.within(ws_view(off[0], B * N, (B, N)), rs_, "scores")
        fig["loss"] = ck.within(ws_view(off[3], 1, ()), ref_loss, "loss")
        for k in ("text.conv.weight", "text.conv.bias", "conv.fc.weight", "conv.fc.bias"):
            ck.that(float(g64[k].abs().max()) > 0, "the oracle's grad %s is all zero" % k)
            fig["grad " + k] = ck.within(named[k].grad, g64[k], "grad " + k)
        try:
            assert_storage_pads_zero(net)
        except AssertionError as e:
            ck.bad.append(str(e))
    # ---- e: one fused step (launch + Adam)
    if "e" in checks and g64 is not None:
        trainable = {k: v for k, v in p.items() if k in g64}
        adam = O.AdamState(trainable)
        if inbatch:  # new negatives are drawn whatever the batch: a new batch, the oracle's own decisions
            u, pos_items, neg_items, r = bt.draw()
            plan.step(*on_gpu(u, pos_items, neg_items))
            torch.cuda.synchronize()
            ck.that(torch.equal(plan.neg_item.cpu().long(), r), "step: in-batch draws differ from numpy")
            pos, neg = bt.literal(pos_items, neg_items)
            pt, nt = toks[pos_items], toks[neg_items.reshape(-1)].reshape(B, N, T)
            ref_loss, g64, _ = TO.loss_and_grads(p, {k: v.clone() for k, v in b.items()}, u, pos, neg, pt, nt, PAD)
        else:        # the same batch: the same forward and gradients, checked above
            plan.step(*on_gpu(u, pos_items, neg_items))
            torch.cuda.synchronize()
        fig["step loss"] = ck.within(ws_view(off[3], 1, ()), ref_loss, "step loss")
        adam.step(trainable, g64, LR)
        opt.flush()
        torch.cuda.synchronize()
        sd = net.state_dict()
        for k in ("text.conv.weight", "text.conv.bias"):
            diff = float((sd[k].detach().double().cpu() - trainable[k]).abs().max())
            tol = 2 * LR + 1e-4 * float(trainable[k].abs().max())
            print("  %-40s %.3e off after the step (allowed %.3e)" % (k, diff, tol))
            ck.that(diff <= tol, "%s after the step: %.3e off (allowed %.3e)" % (k, diff, tol))
        ck.that(torch.equal(sd["text.embeddings.weight"].cpu().double(), words64), "the frozen word vectors moved")
    plan.close()
    print("  figures %s" % {k: "%.2e" % v for k, v in fig.items()})
    ck.done()
    return fig


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_text_step_against_oracle(case):
    run_case(case)


# ------------------------------------------------------------------------------------ eval tower
EVAL_ROWS = [c for c in C.CASES[:9] if c[3] in (17, 128)]


@pytest.mark.parametrize("case", EVAL_ROWS, ids=C.case_id)
def test_text_eval_tower_against_oracle(case):
    """DCUENet.item_features (running BN statistics) at M = 1 and M = 130 at the widths of the T = 17
    row and of both T = 128 rows (the full kernel at TBW 8 and the chunked <8,1>): within 1e-4 of the
    fp64 oracle's largest feature. Random gamma, beta and running statistics, so eval BatchNorm is not
    the identity."""
    from oracle import text_oracle as TO
    assert len(EVAL_ROWS) == 3
    layout, B, N, T, td, wd, V = case
    net, p, b, toks = build(case)
    gen = torch.Generator().manual_seed(11)
    sd = {}
    for k in p:
        if ".bn" in k:
            p[k] = sd[k] = ((0.5 + torch.rand(p[k].shape, generator=gen)) if k.endswith("weight") else
                            0.3 * torch.randn(p[k].shape, generator=gen)).float().double()
    for k in b:
        if k.endswith("running_mean"):
            b[k] = sd[k] = (0.3 * torch.randn(b[k].shape, generator=gen)).float().double()
        elif k.endswith("running_var"):
            b[k] = sd[k] = (0.5 + torch.rand(b[k].shape, generator=gen)).float().double()
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    net.eval()
    X, _ = _tracks()
    ck = _Checks(C.case_id(case))
    for M in (1, 130):
        items = torch.randint(0, N_TRACKS, (M,), generator=gen)
        with torch.no_grad():
            f = net.item_features(X[items].to(DEV), toks[items].to(DEV))
            ref = TO.item_tower(p, b, X[items].double(), toks[items], PAD, train=False).reshape(M, D)
        ck.within(f.reshape(M, -1)[:, :D], ref, "eval features at M = %d" % M)
    ck.done()


# ------------------------------------------------------------------------------ sentence content
def content_tokens(T, V, toks):
    """The first 18 tracks' rows rewritten: 0 all PAD, 1 BOS + EOS only, 2-5 full length without PAD
    (no BOS / EOS either), 6-8 PAD inside the sentence, 9-11 left padding, 12 a single word after left
    padding at t = T - 1, 13 a single word at t = 0; the rest as drawn (right padding)."""
    toks = toks.clone()
    gen = torch.Generator().manual_seed(23)

    def wordsn(n):
        return torch.randint(3, V, (n,), generator=gen, dtype=torch.int32)

    toks[0] = PAD
    toks[1] = PAD
    toks[1, 0], toks[1, 1] = 1, 2
    for i in range(2, 6):
        toks[i] = wordsn(T)
    for i in range(6, 9):
        toks[i] = wordsn(T)
        toks[i, 0], toks[i, T - 1] = 1, 2
        toks[i, 3 + i] = PAD
        toks[i, 1 if i == 6 else 5] = PAD
    for i in range(9, 12):
        toks[i] = wordsn(T)
        toks[i, :i - 5] = PAD
        toks[i, i - 5], toks[i, T - 1] = 1, 2
    toks[12] = PAD
    toks[12, T - 1] = int(wordsn(1))
    toks[13] = PAD
    toks[13, 0] = int(wordsn(1))
    return toks


def test_sentence_content():
    """Rows no other test holds, at the 18-item row's widths under checks a-d: an all-PAD row (s = 0,
    tidx 255, no gradient, everything finite), BOS + EOS only, full-length rows, PAD inside a sentence
    and on the left (the PAD row's word vector enters its neighbours' windows), and maxima at t = 0 and
    t = T - 1 (verified on the oracle)."""
    layout, B, N, T, td, wd, V = ROW18
    from oracle import text_oracle as TO
    toks = content_tokens(T, V, TO.sentences(torch.Generator().manual_seed(100 + T), N_TRACKS, T, V, PAD, min_len=1))
    pick = (torch.arange(B), torch.arange(B, B * (1 + N)).reshape(B, N))

    def expect(dec, near, zm, tok):
        assert bool((tok[0] == PAD).all()) and bool((dec[0] == 255).all()), "the all-PAD row has a decision"
        assert bool((tok[2:6] != PAD).all()), "the full-length rows hold PAD"
        firm = torch.where(near, torch.full_like(dec, 254), dec)
        assert int((firm[2:6] == 0).sum()) > 0 and int((firm[2:6] == T - 1).sum()) > 0, \
            "no full-length row has a maximum at t = 0 and one at t = T - 1"
        assert int((firm[12] == T - 1).sum()) > 0 and int((firm[13] == 0).sum()) > 0, "the single-word rows are off"
        assert int((firm[9:12] != 255).sum()) > 0 and bool((firm[9][firm[9] < 254] >= 4).all()), "left padding is off"

    run_case(ROW18, cid="sentence-content", toks=toks, pick=pick, checks="abcd", expect=expect)


# --------------------------------------------------------------------------------- first maximum
def tie_case(T):
    return ("catalogue", 3, 5, T, 100, 64, 60)


def run_ties(T):
    """Taps 0 and 2 of half the channels zeroed and sentences over five words: those channels' z
    depends on the position's word alone, so it ties exactly wherever a word repeats, in the oracle
    and on the GPU (a zero weight adds an exact zero). The first of the tied positions must win; taps
    0 and 2 of dW -- the chosen position's neighbours -- show which one did (check c on the oracle's
    route)."""
    case = tie_case(T)
    layout, B, N, _, td, wd, V = case
    gen = torch.Generator().manual_seed(31)
    toks = torch.randint(3, 8, (N_TRACKS, T), generator=gen, dtype=torch.int32)
    toks[::3, 0] = 1  # a third of the rows as BOS + words + EOS + PAD
    for i in range(0, N_TRACKS, 3):
        L = int(torch.randint(T // 2, T - 1, (1,), generator=gen))
        toks[i, L] = 2
        toks[i, L + 1:] = PAD

    def edit(p):
        p["text.conv.weight"][::2, :, 0] = 0
        p["text.conv.weight"][::2, :, 2] = 0

    def expect(dec, near, zm, tok):
        top = zm.max(dim=2)
        tied = ((zm == top.values.unsqueeze(2)) & torch.isfinite(zm)).sum(dim=2)
        n = int(((tied > 1) & (top.values > 0) & ~near).sum())
        print("  %d (item, channel) pairs with an exact tie at a positive maximum" % n)
        assert n >= 100, "the premise fails: %d exact ties" % n
        live = torch.isfinite(top.values)
        assert torch.equal(top.indices[live], first_max(zm)[1][live]), "torch's max does not return the first index"

    return run_case(case, cid="first-maximum-T%d" % T, toks=toks, edit=edit, checks="abcd", oracle_route=True,
                    expect=expect)


def test_first_maximum_on_exact_ties():
    """The documented first-maximum rule, observed: with the defaults (one workgroup per item and
    column block: the tie is settled in a lane's position order and across the wave's four row groups)
    ..."""
    assert "DCUE_TEXT_PARTS" not in os.environ and "DCUE_TEXT_FWD" not in os.environ
    run_ties(17)


def test_first_maximum_across_position_parts():
    """... and with the positions split over two workgroups merged through tickets (DCUE_TEXT_PARTS=2,
    read once per process: a child process) at T = 32, where a tie between the halves is settled by
    the merge."""
    env = dict(os.environ, DCUE_TEXT_PARTS="2")
    env.pop("DCUE_TEXT_FWD", None)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "text_shapes_worker.py"), "32"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout[-6000:])
    assert p.returncode == 0, "DCUE_TEXT_PARTS=2 failed:\n%s" % p.stdout[-6000:]
    assert "text ties ok: T 32 parts 2" in p.stdout


# ------------------------------------------------------------------------------ word-vector range
def _scaled(f):
    return lambda w: w * f


def _one_big_row(w):
    w = w.clone()
    w[5] *= 2.0 ** 12
    return w


WORD_TABLES = {"2^-12": _scaled(2.0 ** -12), "2^12": _scaled(2.0 ** 12), "one-row-2^12": _one_big_row}


@pytest.mark.parametrize("name", list(WORD_TABLES))
def test_word_vector_range(name):
    """The split-f16 scale words_exp against word tables whose magnitude is not about 1, at the
    18-item row's widths under checks a-c: the whole table scaled by 2^-12 and by 2^12 (words_exp
    moves, nothing else should), and one word 2^12 times the others in a third of the sentences --
    there check a holds item by item, each against its own max |s|, so an ordinary sentence may not
    lose its low bits to the scale the large word sets."""
    from dcrecommend import _native as nat
    from oracle import text_oracle as TO
    layout, B, N, T, td, wd, V = ROW18
    words = WORD_TABLES[name]
    toks = TO.sentences(torch.Generator().manual_seed(100 + T), N_TRACKS, T, V, PAD, min_len=1)
    big = name.startswith("one")
    if big:
        toks[::3, 1] = 5  # the large word, in a third of the sentences (position 1: inside every sentence)
    torch.manual_seed(0)
    w = words(TO.init_params(D, H, E, N_USERS, td, wd, V)[0]["text.embeddings.weight"])
    ex = nat.words_exponent(w)
    top = float(w.abs().max()) * 2.0 ** ex
    print("words_exp %d: max |word| %.3e -> %.1f" % (ex, float(w.abs().max()), top))
    assert 2.0 ** 13 <= top < 2.0 ** 15
    if not big:  # the exponent moves by the table's scale
        assert ex == nat.words_exponent(w / words(torch.ones(()))) - (12 if name == "2^12" else -12)

    def expect(dec, near, zm, tok):
        if big:
            share = float((tok == 5).any(dim=1).double().mean())
            assert 0.2 <= share <= 0.6, "the large word is in %.2f of the batch's sentences" % share

    # (2^-12: z is the bias plus a small term, so its maxima lie close together against max |z| -- a
    # batch inside the near-tie cap is about one in eight)
    run_case(ROW18, cid="word-range-" + name, toks=toks, words=words, checks="abc", per_item=big, expect=expect,
             tries=64)
