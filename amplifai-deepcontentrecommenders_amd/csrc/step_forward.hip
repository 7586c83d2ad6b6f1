// The forward of a step, and the eval towers, mirroring the reference's (nn/dcue.py:202-210):
//   forward   bn0 stats -> [conv_l (BN_{l-1} fused in its load) -> BN_l stats] x5 -> fc ->
//             user tower -> cosine scores + hinge loss                (dcue/dcue.py:70-108)
#include "step_internal.h"

namespace dcue {

TextBranch text_branch(const Ctx& c, const dcue_tracks* t) {
  const dcue_dims* d = &c.m->dims;
  TextBranch tb;
  tb.tokens = t->tokens;
  tb.words = c.m->words;
  tb.words_exp = c.m->words_exp;
  tb.wpack16 = c.m->wpack + wpack_layout(d).text_f16;
  tb.bias = c.P(SEG_TX_B);
  tb.T = d->text_len; tb.E = d->word_dim; tb.EP = st_word(d); tb.C = c.CT; tb.Creal = d->text_dim;
  tb.pad = d->text_pad;
  return tb;
}

namespace {

// the text branch's forward with the workspace's position-part merge buffers (DCUE_TEXT_PARTS=2)
int text_forward(const Ctx& c, const Ws& w, const dcue_tracks* t, const int32_t* item_track, int M, hipStream_t s) {
  TextBranch tb = text_branch(c, t);
  tb.ticket = w.tticket;
  tb.part = w.tpart;
  return launch_text_fwd(tb, item_track, M, w.xfc, c.FI, w.tidx, s);
}

// the user tower's two GEMMs: h1 = relu(E[u]) W1^T + b1, uf = relu(h1) W2^T + b2
void user_gemms(const Ctx& c, const Ws& w, const int64_t* users, int B, float* uf_out, TGemmArgs* g1, TGemmArgs* g2) {
  *g1 = gemm_args(B, c.E, c.E, c.m->emb, c.E, 1, c.P(SEG_L1_W), 1, c.E, w.h1, c.E);
  g1->arow = users;
  g1->bias = c.P(SEG_L1_B);
  *g2 = gemm_args(B, c.D, c.E, w.h1, c.E, 1, c.P(SEG_L2_W), 1, c.E, uf_out ? uf_out : w.uf, c.D);
  g2->bias = c.P(SEG_L2_B);
}

// the prologue kernel's batch part: copy counts and, for small gather batches, the copy lists
StepPrologue count_args(const dcue_batch* b, const Ws& w) {
  StepPrologue p = {};
  p.B = b->n_rows; p.N = b->n_neg; p.M = b->n_items;
  p.gather = b->layout == DCUE_LAYOUT_GATHER;
  p.neg = const_cast<int32_t*>(b->neg_item);
  p.counts = w.counts;
  if (copy_lists(b)) {
    p.copy_ptr = w.copy_ptr;
    p.copy_idx = w.copy_idx;
  }
  return p;
}

// counts (+ copy lists) of a batch issued outside a plan: the prologue kernel without draws, so
// eager steps and plan replays sum the item gradients in the same order
int batch_counts(const dcue_batch* b, const Ws& w, hipStream_t s) {
  if (!copy_lists(b)) return launch_item_counts(b, w.counts, s);
  return launch_step_prologue(count_args(b, w), s);
}

}  // namespace

int user_forward(const Ctx& c, const Ws& w, const int64_t* users, int B, float* uf_out, hipStream_t s) {
  TGemmArgs g1, g2;
  user_gemms(c, w, users, B, uf_out, &g1, &g2);
  TRY(launch_tgemm(1, 0, g1, s));
  return launch_tgemm(1, 0, g2, s);
}

int item_forward(const Ctx& c, const Ws& w, const dcue_tracks* t, const int32_t* item_track, int M,
                 double copies, bool train, const float* counts, float* f_out, hipStream_t s,
                 const ItemFwdOpts& io) {
  const dcue_model* m = c.m;
  if (c.text && !t->tokens) return DCUE_ERR_INVALID;
  const int src = track_src(t);
  // one BN's finalize/publish record for its first consumer (train) -- bnacc.h
  auto bn_of = [&](int l) {
    BnPublish p = {};
    if (!train || !c.bn) return p;  // eval / no BatchNorm: consumers read the mean / a arrays
    p.acc = bn_acc(w.bnacc, w.cmax, l);
    p.count = copies * (l == 0 ? kFrames : layer_geom(l).lp);
    p.inv_count = 1.0 / p.count;
    p.gamma = c.gamma(w, l);
    p.beta = c.beta(w, l);
    p.mean = w.mean[l]; p.invstd = w.invstd[l]; p.a = w.a[l];
    p.beta_out = w.bcp[l];
    p.rmean = c.rmean(l); p.rvar = c.rvar(l); p.nbt = m->bn_batches + l;
    p.C = bn_channels(&m->dims, l);
    return p;
  };
  // the forward sums and value ranges start cleared (train: by the step prologue, or here). The text
  // branch's position-merge tickets sit at the end of that part; when the branch runs on a side
  // stream (text_join) that stream clears them itself, in its own order (forward_impl), so this
  // clear cannot land between its parts' arrivals
  if (!train || !io.acc_cleared)
    DCUE_HIP_CHECK(hipMemsetAsync(w.bnacc, 0, sizeof(unsigned long long) * (w.nfwd - (io.text_join ? w.ntick : 0)), s));
  if (!c.bn) {  // mean 0, invstd = a = 1, beta 0 for every layer: the BN-free towers
    TRY(launch_bn_identity(w.mean, w.invstd, w.a, w.ones, w.zeros, w.cmax, c.H, c.D, s));
  } else if (!train) {
    for (int l = 0; l < 6; ++l)
      TRY(launch_bn_eval(bn_channels(&m->dims, l), c.P(seg_bn_w(l)), c.rmean(l), c.rvar(l), w.mean[l],
                         w.invstd[l], w.a[l], s));
  }
  if (c.bn && train) {
    if (io.clear_bn0 && !io.stats_done) {  // sums of a batch announced ahead but not the one launched
      DCUE_HIP_CHECK(hipMemsetAsync(bn_acc(w.bnacc, w.cmax, 0), 0, sizeof(unsigned long long) * 2 * w.cmax * 2, s));
      DCUE_HIP_CHECK(hipMemsetAsync(rng_at(w, 0), 0, sizeof(unsigned) * 2 * kRngC, s));
    }
    if (!io.stats_done)  // else computed one step ahead into this accumulator block (plans)
      TRY(launch_input_stats(src, t->data, item_track, counts, M, bn_acc(w.bnacc, w.cmax, 0), rng_at(w, 0), s));
  } else {  // eval, BN-free towers: only the raw input's range, for conv 1's split
    TRY(launch_input_stats(src, t->data, item_track, nullptr, M, nullptr, rng_at(w, 0), s));
  }
  // SyncBN: each layer's batch sums over every rank before their first consumer (the next launch on
  // this stream finalizes them); the counts are already the global ones (forward_impl)
  const bool sync = train && c.bn && io.sync_bn;
  if (sync) TRY(comm_allreduce_u64(io.sync_bn, bn_acc(w.bnacc, w.cmax, 0), 4L * w.cmax, s));
  const WpackLayout wl = wpack_layout(&m->dims);
  auto rows_args = [&](int l) {
    RowsArgs a = {};
    a.src = l == 1 ? t->data : (const void*)w.y[l - 1];
    a.item_track = item_track;
    a.in_mean = w.mean[l - 1];
    a.in_a = w.a[l - 1];
    a.in_beta = c.beta(w, l - 1);
    a.in_bn = bn_of(l - 1);
    a.counts = counts;
    a.wpack = m->wpack + wl.conv_fwd[l];
    a.wpack16 = reinterpret_cast<const uint4*>(m->wpack + wl.conv_f16[l]);
    a.bias = c.P(seg_conv_b(l));
    a.out = w.y[l];
    a.out_idx = w.idx[l];
    a.out_acc = train ? bn_acc(w.bnacc, w.cmax, l) : nullptr;
    a.in_range = rng_at(w, l - 1);
    a.out_range = rng_at(w, l);
    a.M = M;
    a.nout = l == 5 ? c.D : c.H;
    if (l == 1) a.start_sig = io.start_sig;  // (plans: the step's start, for the side streams)
    if (l == 2 && train) {  // conv 2's input-gradient operands, left by the split plans' late Adam
      a.rp = pack_seg(m, c.poff, 2);
      a.rp.fwd = a.rp.f16 = -1;
      a.rp_src = c.P(seg_conv_w(2));
      a.rp_wpack = m->wpack;
    }
    return a;
  };
  for (int l = 1; l <= 5; ++l) {
    RowsArgs a = rows_args(l);
    // the previous step's late-segment Adam (split plans, StepOpts::dense_split) ran on the user stream:
    // conv 2 is the first kernel on this one to read those parameters. It polls a signal itself
    if (l == 2) TRY(wait_or_poll(s, io.before_l2, &a.wait));
    if (l == 2 && train) TRY(debug_delay(DCUE_SITE_CONV2, s));
    TimerScope tsc;
    TRY(timer_begin(&tsc, l == 1 ? DCUE_TIMED_CONV1_FWD : -1, s));
    TRY(launch_conv_fwd(l, l == 1 ? kMels : c.H, l == 1 ? src : SRC_ACT, a, s));
    TRY(timer_end(&tsc));
    TRY(probe(PR_Y1 + l - 1, w.y[l], (long)M * layer_geom(l).lp * a.nout, s));
    if (sync) TRY(comm_allreduce_u64(io.sync_bn, bn_acc(w.bnacc, w.cmax, l), 4L * w.cmax, s));
    if (l == 1 && io.after_l1) TRY(io.after_l1(io.hook));
  }
  // the fc: f = [its input] W^T + b, the input xfc, or in the BN tower y5 with BN5 applied at the load
  const bool cat = c.res || c.text;
  TGemmArgs g = gemm_args(M, c.D, c.FI, cat ? w.xfc : w.y[5], c.FI, 1, c.P(SEG_FC_W), 1, c.FI, f_out ? f_out : w.f, c.D);
  g.bias = c.P(SEG_FC_B);
  if (cat) {  // fc on [tp1, tp2, tp3, tp4, bn5(y5)] (truedcuemel1dres.py:93-97) or [s, bn5(y5)]
    TRY(launch_timepool(w.y, w.mean, w.a, c.bn ? c.P(seg_bn_b(1)) : nullptr, c.bn ? c.P(seg_bn_b(2)) : nullptr,
                        c.bn ? c.P(seg_bn_b(3)) : nullptr, c.bn ? c.P(seg_bn_b(4)) : nullptr,
                        c.bn ? c.P(seg_bn_b(5)) : nullptr, bn_of(5), M, c.H, c.res ? c.HL : 0, c.D, c.off5,
                        c.FI, w.xfc, s));
    if (c.text && io.text_join) {  // the text branch ran on a side stream (forward_impl): join it
      TRY(io.text_join(io.hook));
    } else if (c.text) {
      TimerScope tsc;
      TRY(timer_begin(&tsc, DCUE_TIMED_TEXT_FWD, s));
      TRY(text_forward(c, w, t, item_track, M, s));
      TRY(timer_end(&tsc));
    }
    TRY(launch_tgemm(0, 0, g, s));
    return probe(PR_F, g.C, (long)M * c.D, s);
  }
  // fc on BN5(y5): f = bn5(y5) W^T + b   (truedcuemel1dbn.py:65,101; FI = D)
  g.amean = w.mean[5]; g.aa = w.a[5]; g.abeta = c.beta(w, 5);
  g.abn = bn_of(5);
  TRY(launch_tgemm(2, 0, g, s));
  return probe(PR_F, g.C, (long)M * c.D, s);
}

namespace {

// One forward_impl call's state. The side queue is the last member: the closure posted to it references
// the others, and its destructor waits for it first, on every return path.
struct Forward {
  const dcue_model* m;
  const dcue_batch* b;
  const dcue_tracks* t;
  const StepOpts& o;
  hipStream_t s;
  bool train;
  Ctx c;
  Ws w;
  SidePool* sp;
  hipStream_t su;
  Edge start;       // the step's start on `s`: the plan's, or an event recorded here
  bool split_fwd;   // DCUE_USER_FWD=split: k_emb_sync + two k_tgemm (A/B)
  bool uf_sig;      // plans: the score kernel waits for the user tower on the device (uf_wait)
  DevWait uf_wait;
  hipEvent_t ev_uf, ev_tx;  // the ends of the user tower and of the text branch
  int ust;
  uint64_t useq;
  SideQueue side{};
  int run(float margin), score(float margin), user_part(), text_part();
  int post_user() {  // with the side-issue thread (side.hip) the user part is issued there
    useq = side.run([this] { return user_part(); }, &ust);
    return ust;
  }
  // the fc waits for the text branch: its launch issued (the side thread's part done), then its end
  int text_join() {
    if (!side.threaded()) TRY(user_part());
    TRY(side.wait(useq));
    return wait_point(s, ev_tx);
  }
};

// the user tower on su: emb rows brought up to date, then the two GEMMs (+ the text branch, the
// rolling flush slice)
int Forward::user_part() {
  DevWait ustart{};  // k_user_fwd polls a start signal itself; the three-launch form follows a relay
  if (split_fwd)
    TRY(wait_edges(su, &start, 1));
  else
    TRY(wait_or_poll(su, start, &ustart));
  HPROF("capi:5");
  TRY(debug_delay(DCUE_SITE_USER_FWD, su));
  // The rows' sync and the two GEMMs in one launch (k_user_fwd); DCUE_USER_FWD=split issues them
  // as three (k_emb_sync, one workgroup per row, then two k_tgemm) -- A/B and the schedule test.
  auto launch = [&]() -> int {
    if (split_fwd) {
      if (m->emb_step) TRY(launch_emb_sync(m, b->users, b->n_rows, su));
      return user_forward(c, w, b->users, b->n_rows, nullptr, su);
    }
    TGemmArgs g1, g2;  // (the fused launch polls ustart and signals uf from its own workgroups: DevWait)
    user_gemms(c, w, b->users, b->n_rows, nullptr, &g1, &g2);
    return launch_user_fwd(m, g1, g2, b->users, b->n_rows, su, uf_sig ? o.sig + kSigUf : nullptr, ustart);
  };
  TimerScope tsu;  // (the fused launch is timed live: DCUE_TIMED_USER_FWD)
  TRY(timer_begin(&tsu, split_fwd ? -1 : DCUE_TIMED_USER_FWD, su));
  if (tsu.b && !tsu.capturing) {  // a timed launch: the timer's stop event is its end
    TRY(launch());
    ev_uf = tsu.b;
  } else {  // (untimed, or a captured plan: its timer node follows the launch)
    ForkAfter fk(sp, su, &ev_uf);
    TRY(launch());
    HPROF("capi:7");
    TRY(fk.done());
    HPROF("capi:8");
  }
  TRY(timer_end(&tsu));
  if (uf_sig && split_fwd) TRY(launch_signal(o.sig + kSigUf, uf_wait.val, su));
  TRY(probe(PR_H1, w.h1, (long)b->n_rows * c.E, su));
  TRY(probe(PR_UF, w.uf, (long)b->n_rows * c.D, su));
  if (c.text) TRY(text_part());
  if (o.flush_slice_step >= 0 && m->emb_step) TRY(launch_emb_flush_rows(m, o.flush_slice_step, su));
  return DCUE_OK;
}

// The text branch: the item tower's fc input columns [0, C_s), beside its convs on wgrad stream 1 (the
// user stream holds the user tower's ≈65 µs): after the launch's start point (the items) and the previous
// step's late Adam (its weights); its text weight gradient, which read xfc / tidx, ran on this stream
int Forward::text_part() {
  hipStream_t stx = sp->st[2];
  // Not the edge's own choice: the late Adam's signal is waited for only where the start is a signal
  // too, in the relay that start needs anyway; beside a start event its event costs no launch
  Edge after[2] = {start, o.late};
  if (!start.dev()) after[1].sig = DevWait{};
  TRY(wait_edges(stx, after, 2));
  // the position-merge tickets: cleared by the step prologue (plans, before the start), else here --
  // item_forward's clear on the caller's stream leaves them out
  if (!(train && o.prologue_done) && w.ntick)
    DCUE_HIP_CHECK(hipMemsetAsync(w.tticket, 0, sizeof(unsigned long long) * w.ntick, stx));
  TRY(debug_delay(DCUE_SITE_TEXT_FWD, stx));
  TimerScope tsc;
  TRY(timer_begin(&tsc, DCUE_TIMED_TEXT_FWD, stx));
  auto launch = [&] { return text_forward(c, w, t, b->item_track, b->n_items, stx); };
  if (tsc.b && !tsc.capturing) {  // a timed launch: the timer's stop event is its end
    TRY(launch());
    ev_tx = tsc.b;
  } else {
    ForkAfter fk(sp, stx, &ev_tx);
    TRY(launch());
    TRY(fk.done());
  }
  return timer_end(&tsc);
}

int Forward::score(float margin) {
  if (!o.fuse_score) {
    if (uf_sig) return DCUE_ERR_INVALID;  // (device waits: plans, which fuse the score backward)
    return launch_score_fwd(w.uf, w.f, b, c.D, margin, w.scores, w.cosv, w.norms, w.hinge, w.loss, w.dhinge, s);
  }
  // a fork point after the score kernel only for a caller that asks for one (else nothing is bound): a
  // launch-bound event costs the chain a ≈6 µs gap (the backward's side work waits for dgrad 4 instead)
  const int B = b->n_rows, N = b->n_neg;
  hipEvent_t ev = nullptr;
  ForkAfter fk(sp, s, o.score_done ? &ev : nullptr);
  TRY(launch_score_fused(w.uf, w.f, b, c.D, margin, w.scores, w.cosv, w.norms, w.rowsum, w.du, w.dfcopy, s,
                         uf_wait));
  TRY(fk.done());
  if (o.score_done) {
    HPROF("capi:10");
    *o.score_done = ev;
  }
  TRY(probe(PR_SCORES, w.scores, (long)B * N, s));
  TRY(probe(PR_DU, w.du, (long)B * c.D, s));
  return probe(PR_DFCOPY, w.dfcopy, (long)B * (N + 1) * c.D, s);
}

int Forward::run(float margin) {
  // SyncBN: BatchNorm normalises over every rank's copies (same B, N on each rank)
  const double copies = (double)b->n_rows * (1 + b->n_neg) * (o.sync_bn ? comm_world(o.sync_bn) : 1);
  sp = side_pool();
  if (!sp) return DCUE_ERR_HIP;
  su = sp->st[0];
  // the user tower runs beside the item tower, whose chain is issued first. Plans in the steady state:
  // conv 1 raises the start signal and the side streams wait for it on the device; no event is recorded
  start = o.start;
  if (capturing_step()) start.sig = DevWait{};
  if (!start.ev && !start.dev()) TRY(fork_point(sp, s, &start.ev));
  HPROF("capi:3");
  if (!o.prologue_done) TRY(batch_counts(b, w, s));
  HPROF("capi:4");
  static const bool split = env_is(getenv("DCUE_USER_FWD"), 's');
  split_fwd = split;
  uf_sig = o.sig != nullptr && !capturing_step();
  // the fused launch signals from its own workgroups; the three-launch form through k_signal
  if (uf_sig)
    uf_wait = next_signal(o.sig, o.sig_issued, kSigUf, split_fwd ? 1u : (unsigned)user_fwd_blocks(b->n_rows));
  // (a part that waits for the start signal is enqueued only after conv 1, which raises it, has been)
  const bool post_after_l1 = start.dev() && side.threaded();
  if (side.threaded() && !post_after_l1) TRY(post_user());
  // the previous split step's late Adam: one wait before conv 1 (DCUE_LATE_WAIT=conv1), else before
  // conv 2 (under an exchange the late Adam follows the all-reduce: it keeps its wait before conv 2)
  const bool late_first = o.late.ev && late_wait_at_conv1() && !o.comm;
  if (late_first) TRY(wait_point(s, o.late.ev));
  ItemFwdOpts io;
  io.acc_cleared = o.prologue_done;
  io.stats_done = o.input_stats_done && o.prologue_done;
  io.clear_bn0 = o.clear_bn0;
  if (!late_first) io.before_l2 = o.late;
  if (capturing_step()) io.before_l2.sig = DevWait{};
  io.sync_bn = o.sync_bn;
  if (start.dev()) io.start_sig = const_cast<unsigned*>(start.sig.flag);
  io.hook = this;
  if (post_after_l1) io.after_l1 = [](void* f) { return static_cast<Forward*>(f)->post_user(); };
  // the text branch runs on a side stream beside the audio convs; its join issues the user part
  if (c.text) io.text_join = [](void* f) { return static_cast<Forward*>(f)->text_join(); };
  TRY(item_forward(c, w, t, b->item_track, b->n_items, copies, train, w.counts, nullptr, s, io));
  if (!side.threaded() && !c.text) TRY(user_part());
  TRY(side.wait(useq));
  if (!uf_sig) TRY(wait_point(s, ev_uf));
  HPROF("capi:9");
  return score(margin);
}

}  // namespace

int forward_impl(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws, size_t ws_bytes,
                 int train, float margin, const StepOpts& o, hipStream_t s) {
  Forward f{m, b, t, o, s, train != 0};
  TRY(init_ctx(&f.c, m));
  HPROF("capi:1");
  TRY(check_batch(b));
  HPROF("capi:2");
  if (!t || !t->data || !ws || !m->emb) return DCUE_ERR_INVALID;
  if (o.fuse_score && !train) return DCUE_ERR_INVALID;
  TRY(step_ws(m, b, ws, ws_bytes, o, &f.w));
  return f.run(margin);
}

int ahead_item_inputs(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, const int32_t* items,
                      const float* counts, unsigned long long* acc, float* xhat0, hipStream_t s) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!c.bn) return DCUE_ERR_UNSUPPORTED;  // bn0-free towers have no input statistics to prepare
  Ws w;
  carve(&m->dims, b->n_rows, b->n_neg, b->n_items, nullptr, &w);
  rebase_acc(&w, acc);
  const int src = track_src(t);
  const int M = b->n_items;
  const double copies = (double)b->n_rows * (1 + b->n_neg);
  TRY(launch_input_stats(src, t->data, items, counts, M, bn_acc(w.bnacc, w.cmax, 0), rng_at(w, 0), s));
  if (wgrad_f16_on()) return DCUE_OK;  // the split-f16 conv-1 weight gradient reads the table itself
  return launch_xhat0(src, t->data, items, M, bn_acc(w.bnacc, w.cmax, 0), copies * kFrames, xhat0, s);
}

int step_prologue(const dcue_model* m, const dcue_batch* b, void* ws, size_t ws_bytes, dcue_mt_state* mt,
                  const int64_t* users_src, const int32_t* items_src, hipStream_t s) {
  Ws w;
  TRY(step_ws(m, b, ws, ws_bytes, StepOpts{}, &w));
  StepPrologue p = count_args(b, w);
  p.mt = mt;
  p.users_dst = const_cast<int64_t*>(b->users); p.users_src = users_src;
  p.items_dst = const_cast<int32_t*>(b->item_track); p.items_src = items_src;
  p.zero = w.bnacc; p.nzero = w.nzero;
  return launch_step_prologue(p, s);
}

}  // namespace dcue
