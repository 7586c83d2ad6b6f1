// The backward of a step, mirroring the reference's (nn/dcue.py:202-210):
//   backward  score grads -> item grads -> fc -> [BN_l bwd sums -> wgrad_l, dgrad_l] l=5..2 ->
//             BN1 -> wgrad_1 (+ bn0 grads without conv1 dgrad) -> user tower -> embedding rows
//   adam      dense params + user table, then weight repack
#include "step_internal.h"

namespace dcue {

// Split plans: where the caller's stream waits for the previous step's late Adam (StepOpts::late).
// Default: before conv 2, and for the next step's prepared inputs (StepOpts::inputs) before the
// conv-1 weight gradient. DCUE_LATE_WAIT=conv1: one wait before conv 1, the late Adam itself waiting
// for the inputs on the user stream first -- one barrier gap fewer on the chain, but conv 1 then starts
// behind the previous step's late Adam: 4-5 µs slower per step (profiles/r04_ab_late_wait.txt).
bool late_wait_at_conv1() {
  static const bool on = [] {
    const char* e = getenv("DCUE_LATE_WAIT");
    return e && e[0] == 'c' && e[4] == '1';
  }();
  return on;
}

namespace {

// One backward_impl call's state. The side queue comes after every member the closures posted to it
// reference: its destructor waits for them first, on every return path.
struct Backward {
  const dcue_model* m;  // backward_impl's arguments
  const dcue_batch* b;
  const dcue_tracks* t;
  const StepOpts& o;
  hipStream_t s;
  float emb_grad_scale;
  Ctx c;
  Ws w;
  int B, N, M, H, D, E;
  double copies;  // copies of the batch BatchNorm normalises over (SyncBN: every rank's)
  bool sync;      // SyncBN: the backward sums are all-reduced before their consumers
  int bn_world, src;
  const int32_t *cptr, *cidx;  // the item gradients' copy lists: the plan's slot's, else the workspace's
  SidePool* sp;
  hipStream_t su, sw[2];  // the user stream, wgrad streams 0 and 1
  bool f16w;              // split-f16 weight gradients (conv_wgrad.hip)
  // split plans: Adam over bn0 / conv 1 / bn1 rides in the bn0-gradient launch (k_bn0_grads_adam), not
  // in one of its own behind it; not under an exchange, whose Adam waits for the all-reduced gradient
  bool fuse_late;
  // split plans without an exchange: the late Adam on the user stream waits for the prepared inputs
  // and the next launch waits for it before conv 1 (late_wait_at_conv1)
  bool inputs_via_late;
  double kd_max;  // the largest copy count of an item, the split-f16 dz bounds' kD factor
  // ev_score: after the score backward, for the xhat0 build of the f32 weight-gradient path only;
  // ev_x0: that build's end, waited for just before the conv-1 weight gradient
  hipEvent_t ev_score, ev_x0;
  // fork[l]: what the consumers of g_l wait for: an event bound to the dgrad that made it (ForkAfter: no
  // record packets on the chain) or, on plans (round 7, DCUE_XQ_FORK: fork_dev), a signal -- dgrad 4 and
  // dgrad 3 count into a word from their own workgroups (RowsArgs::done_sig): no gap behind them
  bool fork_dev;
  Edge fork[6];
  // the ends of the caller's stream, the user stream and wgrad streams 0 and 1; (DCUE_XQ_LATE) the last
  // two as signals: k_signal follows each reduce, and one relay ahead of the late Adam waits for both
  Edge tail[4];
  hipEvent_t joined;    // steps that are not split: wgrad stream 0 once every side stream's part is in
  dcue_adam_args dense;  // split plans: the dense Adam step, either part
  long late;             // the flat buffer's late part starts here (DCUE_SEG_LATE)
  uint64_t ahead_seq;
  int ist;
  SideQueue side{};
  int run(const float* dscores);
  int item_grads(), dgrad_chain(), conv1_tail();  // the chain on the caller's stream
  int user_bwd(), fc_text_wgrad();                               // the side streams' parts
  int layer_wgrads(int lo, int hi, bool with_fc, hipStream_t so, Edge* tl);
  int multi_hi() { return layer_wgrads(3, 5, !c.res && !c.text, sw[0], &tail[2]); }
  int multi_2() { return layer_wgrads(2, 2, false, sw[1], &tail[3]); }
  int join_part(), late_adam(), exchange_tail();  // the step's end
  // posts a side stream's part to the side-issue thread (side.hip; off: runs it here)
  template <int (Backward::*part)()>
  int post() {
    side.run([this] { return (this->*part)(); }, &ist);
    return ist;
  }
  // 1 / BN_l's count; 0: BN backward is the identity
  float inv_n(int l) const { return c.bn ? (float)(1.0 / (copies * layer_geom(l).lp)) : 0.f; }
  // conv layer l's weight-gradient operands but its x source and partial buffers
  WgradArgs wgrad_args(int l) const {
    WgradArgs wa = {};
    wa.item_track = b->item_track;
    wa.g_l = w.g[l]; wa.y_l = w.y[l]; wa.idx_l = w.idx[l];
    wa.mean_l = w.mean[l]; wa.invstd_l = w.invstd[l]; wa.a_l = w.a[l];
    wa.dz_acc = bn_acc(w.bnbacc, w.cmax, l); wa.dgamma = c.dgamma(w, l); wa.dbeta = c.dbeta(w, l);
    wa.invN = inv_n(l);
    wa.bn_world = bn_world;
    wa.counts = w.counts;
    wa.M = M; wa.cout = l == 5 ? D : H; wa.cin = l == 1 ? kMels : H;
    if (f16w) {
      wa.x_range = rng_at(w, l - 1); wa.y_range = rng_at(w, l); wa.g_range = grng_at(w, l);
      wa.kd_max = (float)kd_max * wa.invN;
    }
    return wa;
  }
  int sync_bn_sums(int l) {  // SyncBN: BN_l's backward sums over every rank
    return sync ? comm_allreduce_u64(o.sync_bn, bn_acc(w.bnbacc, w.cmax, l), 4L * w.cmax, s) : DCUE_OK;
  }
};

// user tower (userembedding.py:33-44 backward), the compact embedding rows, and -- when the step
// carries it -- the user table's Adam step. It needs only the score kernel's du, and waits for the dgrad
// chain's first fork point, which the layer 3-5 weight gradients wait for anyway: no extra fork event
int Backward::user_bwd() {
  const Edge after = ev_score ? Edge{ev_score} : fork[3];
  TRY(wait_edges(su, &after, 1));
  HPROF("capi:26");
  TRY(debug_delay(DCUE_SITE_USER_BWD, su));
  {  // two launches of two independent GEMMs each (launch_tgemm_pair; the same blocks as four
    // launch_tgemm calls, so the same bits): (dW2, dh1) from du, then (dW1, de) from dh1
    // dW2[n][k] = sum_b du[b][n] relu(h1)[b][k]; db2[n] = sum_b du[b][n]
    TGemmArgs g = gemm_args(D, E, B, w.du, 1, D, w.h1, E, 1, c.Gd(SEG_L2_W), E);
    g.rowsum = c.Gd(SEG_L2_B);
    // dh1 = (du W2) * (h1 > 0)
    TGemmArgs h = gemm_args(B, E, D, w.du, D, 1, c.P(SEG_L2_W), E, 1, w.dh1, E);
    h.cmask = w.h1; h.smm = E; h.smn = 1;
    TRY(launch_tgemm_pair(g, h, su));
    HPROF("capi:28");
    // dW1[n][k] = sum_b dh1[b][n] relu(E[u_b])[k]; db1[n] = sum_b dh1[b][n]
    g = gemm_args(E, E, B, w.dh1, 1, E, m->emb, E, 1, c.Gd(SEG_L1_W), E);
    g.brow = b->users;
    g.rowsum = c.Gd(SEG_L1_B);
    // de = (dh1 W1) * (E[u_b] > 0)
    h = gemm_args(B, E, E, w.dh1, E, 1, c.P(SEG_L1_W), E, 1, w.de, E);
    h.cmask = m->emb; h.smm = E; h.smn = 1; h.cmrow = b->users;
    TRY(launch_tgemm_pair(g, h, su));
    HPROF("capi:30");
  }
  // the step's end joins the user stream here: its Adam part (and the rolling flush slice) below
  // needs nothing more from this step and runs on into the next one, ordered on this stream
  // deferred user-table Adam with the step (plans): the compact rows and their Adam step in one
  // launch (k_emb_grad_adam: each distinct user's workgroup sums its rows, then steps them)
  const bool emb_fused = o.emb_adam && m->emb_step && o.defer_flush_slice;
  ForkAfter fk(sp, su, &tail[1].ev);
  if (emb_fused)
    TRY(launch_emb_grad_adam(m, o.emb_adam, w.de, b->users, B, emb_grad_scale, su));
  else
    TRY(launch_emb_grad(w.de, b->users, B, E, emb_grad_scale, m->emb_grad, m->emb_slot, m->emb_rows,
                        m->emb_step ? m->emb_log : nullptr, su));
  TRY(fk.done());
  HPROF("capi:31");
  TRY(probe(PR_DE, w.de, (long)B * E, su));
  TRY(probe(PR_G_USER, c.Gd(SEG_L1_W), c.poff[SEG_L2_B + 1] - c.poff[SEG_L1_W], su));
  if (o.emb_adam && !emb_fused) TRY(launch_adam(m, o.emb_adam, c.poff, su, !o.defer_flush_slice));
  HPROF("capi:32");
  return DCUE_OK;
}

// fc weight gradient of the res / text towers: dW[n][k] = sum_m df[m][n] xfc[m][k], db = sum df over the
// concatenated fc input (the other towers' fc rides in the layer 3-5 launch, below)
int Backward::fc_text_wgrad() {
  TRY(wait_point(sw[1], fork[5].ev));
  HPROF("capi:23");
  TRY(debug_delay(DCUE_SITE_FC_WGRAD, sw[1]));
  TGemmArgs g = gemm_args(D, c.FI, M, w.df, 1, D, w.xfc, c.FI, 1, c.Gd(SEG_FC_W), c.FI);
  g.rowsum = c.Gd(SEG_FC_B);
  TRY(launch_tgemm(0, 0, g, sw[1]));
  HPROF("capi:24");
  // the text conv's weight and bias gradients (the max routes each gradient to one position)
  if (c.text)
    TRY(launch_text_wgrad(text_branch(c, t), b->item_track, M, w.dtp, w.tidx, w.twpart, c.Gd(SEG_TX_W),
                          c.Gd(SEG_TX_B), sw[1]));
  TRY(probe(PR_G_FC, c.Gd(SEG_FC_W), c.poff[SEG_FC_B + 1] - c.poff[SEG_FC_W], sw[1]));
  return c.text ? probe(PR_G_FC, c.Gd(SEG_TX_W), c.poff[SEG_TX_B + 1] - c.poff[SEG_TX_W], sw[1]) : DCUE_OK;
}

// Weight gradients of layers hi..lo (+ the fc) in one launch on `so`, + one reduce launch. Layer l's
// reads g_l, which dgrad l+1 produced (fork[l]): layers 5..3 on wgrad stream 0 once dgrad 4 is done;
// layer 2 on wgrad stream 1 (behind xhat0 and the fc weight gradient) once dgrad 3 is, beside dgrad 2
// and the conv-1 tail. *tl: the stream's end, an event bound here or its signal
int Backward::layer_wgrads(int lo, int hi, bool with_fc, hipStream_t so, Edge* tl) {
  TRY(wait_edges(so, &fork[lo], 1));
  TRY(debug_delay(lo == 2 ? DCUE_SITE_WGRAD_2 : DCUE_SITE_WGRAD_HI, so));
  WgradMulti mw = {};
  if (with_fc) {  // fc: dW[n][k] = sum_m df[m][n] bn5(y5)[m][k], db = sum_m df (df final since item_grad)
    const int j = mw.n++;
    mw.layer[j] = 6;
    WgradArgs& wa = mw.a[j];
    wa.xsrc = w.y[5];
    wa.x_mean = w.mean[5]; wa.x_a = w.a[5]; wa.x_beta = c.beta_bwd(w, 5);
    wa.g_l = w.df;
    wa.M = M; wa.cout = D; wa.cin = D;
    wa.wpart = w.wpm[4]; wa.bpart = w.bpm[4];
    if (f16w) {
      wa.x_range = rng_at(w, 5); wa.g_range = grng_at(w, 6);
    }
    mw.nchunk[j] = wgrad_nchunk(6, M, D, D);
    mw.dW[j] = c.Gd(SEG_FC_W);
    mw.db[j] = c.Gd(SEG_FC_B);
  }
  for (int l = hi; l >= lo; --l) {
    const int j = mw.n++;
    mw.layer[j] = l;
    WgradArgs& wa = mw.a[j];
    wa = wgrad_args(l);
    wa.xsrc = w.y[l - 1];
    wa.x_mean = w.mean[l - 1]; wa.x_a = w.a[l - 1]; wa.x_beta = c.beta_bwd(w, l - 1);
    wa.wpart = w.wpm[l - 2]; wa.bpart = w.bpm[l - 2];
    mw.nchunk[j] = wgrad_nchunk(l, M, wa.cout, wa.cin);
    mw.dW[j] = c.Gd(seg_conv_w(l));
    mw.db[j] = c.Gd(seg_conv_b(l));
  }
  ForkAfter fk(sp, so, tl->dev() ? nullptr : &tl->ev);  // (a signalled end binds no event)
  TRY(launch_conv_wgrad_multi(mw, so));
  TRY(fk.done());
  if (tl->dev()) TRY(launch_signal(const_cast<unsigned*>(tl->sig.flag), tl->sig.val, so));
  const int s1 = with_fc ? SEG_FC_B : seg_bn_b(hi);
  return probe(lo == 2 ? PR_G_2 : PR_G_HI, c.Gd(seg_conv_w(lo)), c.poff[s1 + 1] - c.poff[seg_conv_w(lo)], so);
}

// Steps that are not split: the join -- wgrad stream 0 collects the user stream's and wgrad stream 1's
// tails, and the caller's stream waits for it once (each cross-queue wait on a pending event costs the
// waiting queue ≈4 µs, measured; on the side stream that time is slack, on the caller's the step's).
int Backward::join_part() {
  const Edge ends[2] = {tail[1], tail[3]};  // (item-only steps: no user stream's)
  TRY(wait_edges(sw[0], ends, 2));
  return fork_point(sp, sw[0], &joined);
}

// Split plans: the late segments' Adam (every gradient the side streams made) on the user stream once
// the two weight-gradient streams' tails are in -- the user stream's own tail is in stream order. The
// caller's stream does not wait for it (the next forward waits for *late_done before conv 2).
int Backward::late_adam() {
  const Edge ends[2] = {tail[2], tail[3]};
  TRY(wait_edges(su, ends, 2));
  // (the dgrad of conv 2 on the caller's stream may still run: this Adam leaves its packed
  // operands to the next forward of conv 2 -- launch_adam defer_dgrad2; DCUE_LEGACY_ORDERS=1
  // restores the round-4 order, the repack here and no wait: the race tests/test_gpu_races.py shows)
  // (recorded by the plan's prologue closure, posted before this one: FIFO on the side thread)
  if (inputs_via_late && o.inputs.ev) TRY(wait_point(su, o.inputs.ev));
  TRY(debug_delay(DCUE_SITE_LATE_ADAM, su));
  ForkAfter fk(sp, su, o.late_done ? &o.late_done->ev : nullptr);
  TRY(launch_adam(m, &dense, c.poff, su, true, late, -1, !legacy_orders()));
  TRY(fk.done());
  // a one-lane k_signal after the sweep: its 440 workgroups each releasing their own stores (an L2
  // writeback each on gfx950) measured 2-4 us slower per step (profiles/r06_ab_late_signal.txt)
  if (o.late_done && o.late_done->dev())
    TRY(launch_signal(const_cast<unsigned*>(o.late_done->sig.flag), o.late_done->sig.val, su));
  return probe(PR_P_LATE, m->params + late, c.poff[kSeg] - late, su);
}

// df; then the fc input gradient g5 (+ BN5's backward sums)
int Backward::item_grads() {
  const float* rowsum = o.fuse_score ? w.rowsum : nullptr;
  if (c.res || c.text) {  // the fc input gradient split: g5 = df W[:, off5:] (+ BN5's sums) and the
                          // time-pooled blocks' dtp = df W[:, :4H] (text: the text features' df W[:, :C])
    TRY(launch_item_grad(w.dfcopy, b, D, w.df, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rowsum, w.loss,
                         cptr, cidx, nullptr, grng_at(w, 6), s));
    TGemmArgs g = gemm_args(M, D, D, w.df, D, 1, c.P(SEG_FC_W) + c.off5, c.FI, 1, w.g[5], D);
    g.colacc = bn_acc(w.bnbacc, w.cmax, 5); g.xy = w.y[5]; g.xmean = w.mean[5]; g.xinvstd = w.invstd[5];
    g.colmax = grng_at(w, 5);
    TRY(launch_tgemm(0, 0, g, s));
    g = gemm_args(M, c.off5, D, w.df, D, 1, c.P(SEG_FC_W), c.FI, 1, w.dtp, c.text ? c.CT : 4 * c.HL);
    ForkAfter fk(sp, s, &fork[5].ev);
    TRY(launch_tgemm(0, 0, g, s));
    TRY(fk.done());
    if (side.threaded()) TRY(post<&Backward::fc_text_wgrad>());
  } else {  // per-item feature gradients df, then (same kernel) the fc input gradient g5 = df W and BN5's sums
    // (no fork point here: the fc weight gradient waits with the layer 3-5 weight gradients)
    TRY(launch_item_grad(w.dfcopy, b, D, w.df, c.P(SEG_FC_W), w.g[5], bn_acc(w.bnbacc, w.cmax, 5), w.y[5],
                         w.mean[5], w.invstd[5], rowsum, w.loss, cptr, cidx, grng_at(w, 5), grng_at(w, 6), s));
    HPROF("capi:15");
  }
  TRY(probe(PR_DF, w.df, (long)M * D, s));
  TRY(probe(PR_G5, w.g[5], (long)M * D, s));
  return sync_bn_sums(5);
}

// dgrad chain: g_l (+ BN_l sums) -> g_{l-1} (+ BN_{l-1} sums), l = 5..2
int Backward::dgrad_chain() {
  const WpackLayout wl = wpack_layout(&m->dims);
  for (int l = 5; l >= 2; --l) {
    RowsArgs ra = {};
    ra.src = w.g[l]; ra.y_l = w.y[l]; ra.idx_l = w.idx[l];
    ra.mean_l = w.mean[l]; ra.invstd_l = w.invstd[l]; ra.a_l = w.a[l];
    ra.dz_acc = bn_acc(w.bnbacc, w.cmax, l);
    ra.invN = inv_n(l);
    ra.counts = w.counts;
    if (c.res) {  // + d tp_{l-1} / Lp_{l-1} at every position of block l-1 (AvgPool1d backward)
      ra.skip = w.dtp + (l - 2) * c.HL;
      ra.skip_ld = 4 * c.HL;
      ra.skip_n = c.HL;  // storage channels past the reference's H get no skip gradient
      ra.skip_scale = 1.0f / (float)layer_geom(l - 1).lp;
    }
    ra.wpack = m->wpack + wl.conv_bwd[l];
    ra.wpack16 = reinterpret_cast<const uint4*>(m->wpack + wl.conv_f16b[l]);
    // the split-f16 dgrad's dz bound: max |g_l| (the previous dgrad / item gradient), y_l's range
    ra.in_range = grng_at(w, l); ra.y_range = rng_at(w, l);
    ra.kd_max = (float)kd_max * ra.invN;
    ra.out = w.g[l - 1];
    ra.out_acc = bn_acc(w.bnbacc, w.cmax, l - 1);
    ra.oy = w.y[l - 1]; ra.omean = w.mean[l - 1]; ra.oinvstd = w.invstd[l - 1];
    ra.out_grange = grng_at(w, l - 1);  // max |g_{l-1}|: the split-f16 weight gradient's dz bound
    ra.M = M;
    ra.nout = H;
    // a fork point only where a side stream waits (wgrads of layers 3-5 after g_3, of layer 2
    // after g_2): every event bound to a launch costs the chain a gap before its next kernel
    const bool forks = l - 1 == 3 || l - 1 == 2;
    if (forks || l == 2)
      TRY(debug_delay(l - 1 == 3 ? DCUE_SITE_DGRAD_4 : l - 1 == 2 ? DCUE_SITE_DGRAD_3 : DCUE_SITE_DGRAD_2, s));
    hipEvent_t* bind = nullptr;
    if (forks && fork_dev) {
      // the fork point as a signal: the launch's workgroups count into the word, nothing is bound
      const int slot = l - 1 == 3 ? kSigDgrad4 : kSigDgrad3;
      ra.done_sig = o.sig + slot;
      fork[l - 1].sig = next_signal(o.sig, o.sig_issued, slot, (unsigned)conv_dgrad_blocks(l, H, H, M));
    } else if (forks) {
      bind = &fork[l - 1].ev;
    }
    ForkAfter fk(sp, s, bind);  // (null: binds and records nothing)
    TRY(launch_conv_dgrad(l, l == 5 ? D : H, ra, s));
    TRY(sync_bn_sums(l - 1));
    // SyncBN: the weight gradients forked here read the summed BN_{l-1} sums: the fork point is
    // recorded after the exchange instead of bound to the launch
    if (sync && bind) launch_tag().missed = true;
    TRY(fk.done());
    // (the consumers' waits are enqueued after this launch: posted here, FIFO on the side thread)
    if (l - 1 == 3 && side.threaded()) TRY(post<&Backward::multi_hi>());
    // the user tower's backward and a plan's lookahead are issued at the chain's first fork point too
    if (l - 1 == 3 && side.threaded() && !o.item_only) TRY(post<&Backward::user_bwd>());
    if (l - 1 == 3 && o.ahead) {
      const std::function<int(hipEvent_t)>* ah = o.ahead;
      const hipEvent_t e3 = fork[3].ev;
      ahead_seq = side.run([ah, e3]() { return (*ah)(e3); }, &ist);
      TRY(ist);
    }
    if (l - 1 == 2 && side.threaded()) TRY(post<&Backward::multi_2>());
    TRY(probe(PR_G4 + (5 - l), w.g[l - 1], (long)M * layer_geom(l - 1).lp * H, s));
    HPROF("capi:16");
  }
  return DCUE_OK;
}

// the step's tail on the caller's stream: the conv-1 weight gradient, its reduce, and bn0's
// gradients (+ the early segments' Adam), with a fork point after its last kernel (tail[0])
int Backward::conv1_tail() {
  if (ev_x0) TRY(wait_point(s, ev_x0));
  // plans: the next step's prepared inputs. The split-f16 kernel (k_conv_wgrad16t) polls their signal
  // itself instead of a stream wait before it
  Edge inputs = inputs_via_late ? Edge{} : o.inputs;
  if (!f16w || capturing_step()) inputs.sig = DevWait{};
  DevWait inputs_poll{};
  if (inputs.ev) {
    // the host's wait holds for the device-side wait too: the kernel that polls is enqueued only
    // after the side thread has enqueued the launch that signals (enqueue order)
    TRY(side.wait(o.ahead ? ahead_seq : o.wait_inputs_seq));
    TRY(wait_or_poll(s, inputs, &inputs_poll));
  }
  TRY(debug_delay(DCUE_SITE_WGRAD_1, s));
  HPROF("capi:18");
  WgradArgs wa = wgrad_args(1);
  // split-f16 kernels: layer 1 reads the track table itself (bn0 applied at the fill), not xhat0
  wa.xsrc = f16w ? t->data : (const void*)(o.xhat0 ? o.xhat0 : w.xhat0);
  wa.x_mean = w.mean[0];
  wa.x_a = w.invstd[0];
  wa.wpart = w.wpart; wa.bpart = w.bpart;
  wa.wait = inputs_poll;
  const int nch = wgrad_nchunk(1, M, H, kMels);
  if (!f16w) {  // the GEMM reads the pooled BN1 backward, expanded to rows at MFMA time
    TRY(launch_conv1_dx(wa, w.dx1, s));
    wa.g_l = w.dx1;
  }
  TimerScope tsc;
  TRY(timer_begin(&tsc, DCUE_TIMED_CONV1_WGRAD, s));
  HPROF("capi:19");
  TRY(launch_conv_wgrad(src, wa, nch, s));
  HPROF("capi:20");
  TRY(timer_end(&tsc));
  HPROF("capi:21");
  TRY(launch_wgrad_reduce(1, wa.wpart, wa.bpart, nch, H, kMels, c.Gd(seg_conv_w(1)),
                          c.Gd(seg_conv_b(1)), w.G, w.S, s));
  // (split plans without an exchange: nothing waits for the caller stream's tail -- no event bound)
  ForkAfter fk(sp, s, o.dense_split && !o.comm ? nullptr : &tail[0].ev);
  const bool graw = f16w && src == SRC_TRACK_F16;  // G over the raw fp16 input (conv_wgrad.hip)
  const float *mean0 = graw ? w.mean[0] : nullptr, *invstd0 = graw ? w.invstd[0] : nullptr;
  if (fuse_late) {  // split plans: bn0's gradients and Adam over [0, DCUE_SEG_LATE) in one launch
    Bn0Adam ba;
    ba.md = m; ba.poff = c.poff; ba.args = *o.dense_split; ba.bn = c.bn;
    TRY(launch_bn0_grads_adam(w.G, w.S, c.gamma(w, 0), c.beta(w, 0), mean0, invstd0, H, c.dgamma(w, 0),
                              c.dbeta(w, 0), ba, s));
  } else {
    TRY(launch_bn0_grads(w.G, w.S, c.P(seg_conv_w(1)), c.gamma(w, 0), c.beta(w, 0), mean0, invstd0, H,
                         c.Gd(seg_conv_w(1)), c.dgamma(w, 0), c.dbeta(w, 0), c.Gd(seg_conv_b(1)), s));
  }
  TRY(fk.done());
  TRY(probe(PR_G_1, m->grads, late, s));
  return fuse_late ? probe(PR_P_EARLY, m->params, late, s) : DCUE_OK;
}

// Data parallelism, split: each bucket's Adam waits only for its all-reduce (comm_exchange_split): the
// late segments' (every side stream's gradient) on the comm stream, then bn0 / conv 1 / bn1 on this one
// after the early bucket; *late_done is what the next forward's conv 2 waits for, as without an exchange
int Backward::exchange_tail() {
  TRY(side.drain());
  const long n = c.poff[kSeg];
  const hipEvent_t sides[3] = {tail[1].ev, tail[2].ev, tail[3].ev};
  hipEvent_t ld = ring_event(sp);
  TRY(comm_exchange_split(o.comm, m, &dense, c.poff, late, n, sides, 3, ld, s));
  if (o.late_done) o.late_done->ev = ld;
  TRY(launch_adam(m, &dense, c.poff, s, true, 0, late));
  TRY(probe(PR_P_EARLY, m->params, late, s));
  if (o.tails) {  // [1]: the comm stream after the late Adam, which waited for every side stream
    o.tails[0] = tail[0].ev;
    o.tails[1] = ld;
  }
  return DCUE_OK;
}

// Host issue order follows the critical path: the main stream's chain (item grads -> fc -> the dgrad
// chain -> the conv-1 tail) is enqueued first, with a fork point where a side stream waits; the side
// streams' work (user tower, fc and per-layer weight gradients) is posted to the side-issue thread at
// those points -- without it, issued here after the chain -- so issuing it never delays the chain.
int Backward::run(const float* dscores) {
  B = b->n_rows; N = b->n_neg; M = b->n_items;
  H = c.H; D = c.D; E = c.E;
  copies = (double)B * (1 + N) * (o.sync_bn ? comm_world(o.sync_bn) : 1);
  sync = o.sync_bn && c.bn;
  bn_world = sync ? comm_world(o.sync_bn) : 0;
  src = track_src(t);
  if (o.fuse_score && dscores) return DCUE_ERR_INVALID;
  cptr = o.copy_ptr ? o.copy_ptr : (copy_lists(b) ? w.copy_ptr : nullptr);
  cidx = o.copy_ptr ? o.copy_idx : (copy_lists(b) ? w.copy_idx : nullptr);
  if (o.emb_adam && (o.emb_adam->parts & ~DCUE_ADAM_EMBEDDING)) return DCUE_ERR_INVALID;
  sp = side_pool();
  if (!sp) return DCUE_ERR_HIP;
  su = sp->st[0]; sw[0] = sp->st[1]; sw[1] = sp->st[2];
  if (!o.prologue_done)  // the backward sums and the gradient maxima
    DCUE_HIP_CHECK(hipMemsetAsync(w.bnbacc, 0, sizeof(unsigned long long) * (6 * 2 * w.cmax * 2 + kGrngWords), s));
  HPROF("capi:13");
  if (!o.fuse_score && !o.item_only)  // else the fused score kernel (or the MSE head) produced dfcopy
    TRY(launch_score_bwd(w.uf, w.f, b, D, dscores ? dscores : w.dhinge, w.cosv, w.norms, w.du, w.dfcopy, s));
  f16w = wgrad_f16_on();
  if (o.fuse_score && o.score_done && *o.score_done)
    ev_score = *o.score_done;
  else if (!o.xhat0 && !f16w)
    TRY(fork_point(sp, s, &ev_score));
  HPROF("capi:14");
  fuse_late = o.dense_split && !o.comm && o.dense_split->grad_div <= 1.0;
  kd_max = b->layout == DCUE_LAYOUT_GATHER ? 1.0 + (double)B * N : 1.0;
  // the conv-1 weight gradient's X operand, bn0(x) without gamma/beta, materialised once beside the
  // backward chain (it needs only the forward's input statistics) unless a plan prepared it
  if (!o.xhat0 && !f16w) {
    TRY(wait_point(sw[1], ev_score));
    ForkAfter fk(sp, sw[1], &ev_x0);
    TRY(launch_xhat0(src, t->data, b->item_track, M, c.bn ? bn_acc(w.bnacc, w.cmax, 0) : nullptr,
                     copies * kFrames, w.xhat0, sw[1]));
    TRY(fk.done());
  }
  if (c.text && !t->tokens) return DCUE_ERR_INVALID;
  // Which edges are signals (plans); the fork points not with the A/B orders that hand fork[3]'s event
  // on (DCUE_AHEAD_AT=fork, DCUE_SCORE_FORK) or SyncBN. Their counters advance here, before any post.
  const bool plan_sig = o.sig && o.sig_issued && !capturing_step();
  fork_dev = plan_sig && xq_edge_on(XQ_FORK) && !o.ahead && !o.sync_bn && !(o.score_done && *o.score_done) &&
             !o.item_only;
  if (plan_sig && xq_edge_on(XQ_LATE) && o.dense_split && !o.comm) {
    tail[2].sig = next_signal(o.sig, o.sig_issued, kSigWgradHi);
    tail[3].sig = next_signal(o.sig, o.sig_issued, kSigWgrad2);
  }
  inputs_via_late = o.dense_split && !o.comm && o.late_done && late_wait_at_conv1();
  // plans (split, no exchange): the late Adam also signals the next step's conv 2
  if (o.dense_split && !o.comm && o.late_done && o.sig && !capturing_step())
    o.late_done->sig = next_signal(o.sig, o.sig_issued, kSigLate);
  if (o.dense_split) {
    dense = *o.dense_split;
    dense.parts = DCUE_ADAM_DENSE;
  }
  late = c.poff[DCUE_SEG_LATE];

  TRY(item_grads());   // posts the res / text towers' fc weight gradient
  TRY(dgrad_chain());  // posts the layer weight gradients, the user tower's backward and the lookahead
  TRY(conv1_tail());
  HPROF("capi:22");
  if (!side.threaded()) {
    if (c.res || c.text) TRY(fc_text_wgrad());
    TRY(multi_hi());
    TRY(multi_2());
    HPROF("capi:25");
    if (!o.item_only) TRY(user_bwd());
    HPROF("capi:32");
  }
  if (o.dense_split && o.comm) return exchange_tail();
  // the step's end. Split plans: bn0 / conv 1 / bn1 step here unless they rode in the bn0-gradient launch
  if (o.dense_split) {
    TRY(post<&Backward::late_adam>());
    if (!fuse_late) {
      TRY(launch_adam(m, &dense, c.poff, s, true, 0, late));
      TRY(probe(PR_P_EARLY, m->params, late, s));
    }
  } else {
    TRY(post<&Backward::join_part>());
    TRY(side.drain());
    TRY(wait_point(s, joined));
  }
  TRY(side.drain());
  HPROF("capi:36");
  if (o.tails) {  // [1], split steps: the user stream after the late Adam (it waited for the others)
    o.tails[0] = tail[0].ev;
    o.tails[1] = o.dense_split && o.late_done ? o.late_done->ev : joined;
  }
  return DCUE_OK;
}

}  // namespace
int backward_impl(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws, size_t ws_bytes,
                  const float* dscores, float emb_grad_scale, const StepOpts& o, hipStream_t s) {
  Backward bw{m, b, t, o, s, emb_grad_scale};
  TRY(init_ctx(&bw.c, m));
  HPROF("capi:11");
  if (!o.item_only) TRY(check_batch(b));
  HPROF("capi:12");
  if (!t || !t->data || !ws || !m->grads) return DCUE_ERR_INVALID;
  if (!o.item_only && (!m->emb_grad || !m->emb_slot)) return DCUE_ERR_INVALID;
  TRY(step_ws(m, b, ws, ws_bytes, o, &bw.w));
  return bw.run(dscores);
}

}  // namespace dcue
