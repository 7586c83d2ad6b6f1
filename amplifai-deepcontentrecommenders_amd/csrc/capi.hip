// libdcue_hip C ABI: the dims, the parameter / BatchNorm / workspace layouts and the extern "C" entry
// points. The per-step kernel schedule is in step_forward.hip and step_backward.hip, the side streams
// and the orders between streams in streams.hip, plans in plan.hip.
#include <math.h>
#include <string.h>

#include "step_internal.h"

using namespace dcue;

namespace {

int check_dims(const dcue_dims* d) {
  if (!d) return DCUE_ERR_INVALID;
  if (d->conv_hidden <= 0 || d->feature_dim <= 0 || d->user_embdim <= 0 || d->n_users < 0)
    return DCUE_ERR_INVALID;
  // any width up to 256 (run at its storage width, dcue_common.h); the user tower's E up to 1024
  if (d->conv_hidden > 256 || d->feature_dim > 256 || d->user_embdim > 1024) return DCUE_ERR_UNSUPPORTED;
  if (d->tower < DCUE_TOWER_BN || d->tower > DCUE_TOWER_TEXT) return DCUE_ERR_INVALID;
  if (d->tower == DCUE_TOWER_TEXT) {  // text.hip's limits: uint8 argmax positions, float4 word rows
    if (d->text_dim <= 0 || d->word_dim <= 0 || d->text_len < 2 || d->text_pad < 0) return DCUE_ERR_INVALID;
    if (d->text_dim > 256 || d->word_dim > 1024 || d->word_dim % 4 || d->text_len > 128) return DCUE_ERR_UNSUPPORTED;
  }
  return DCUE_OK;
}

long al4(long v) { return (v + 3) & ~3L; }

void param_sizes(const dcue_dims* d, long* sz) {
  const long H = st_hidden(d), D = st_feature(d), E = d->user_embdim;
  const long cin[5] = {kMels, H, H, H, H}, cout[5] = {H, H, H, H, D};
  const long bn = tower_has_bn(d) ? 1 : 0;  // the BN parameters' segments are empty without BN
  int s = 0;
  sz[s++] = bn * kMels;  // bn0.weight
  sz[s++] = bn * kMels;  // bn0.bias
  for (int l = 1; l <= 5; ++l) {
    sz[s++] = cout[l - 1] * cin[l - 1] * layer_geom(l).ks;  // conv.layer{l}.weight
    sz[s++] = cout[l - 1];                                  // conv.layer{l}.bias
    sz[s++] = bn * cout[l - 1];                             // conv.bn{l}.weight
    sz[s++] = bn * cout[l - 1];                             // conv.bn{l}.bias
  }
  sz[s++] = D * fc_in(d);  // conv.fc.weight [d][d] or, res towers, [d][4H + d]
  sz[s++] = D;      // conv.fc.bias
  sz[s++] = E * E;  // user_embd.linear1.weight
  sz[s++] = E;
  sz[s++] = D * E;  // user_embd.linear2.weight
  sz[s++] = D;
  const long CT = st_text(d);  // 0 outside the text tower: empty segments
  sz[s++] = CT * d->word_dim * 3;  // text.conv.weight [C_s][E_w][3]
  sz[s++] = CT;                    // text.conv.bias
}

void param_offsets(const dcue_dims* d, int64_t* off) {
  long sz[kSeg];
  param_sizes(d, sz);
  long o = 0;
  for (int s = 0; s < kSeg; ++s) {
    off[s] = o;
    o = al4(o + sz[s]);
  }
  off[kSeg] = o;
}

void bn_offsets(const dcue_dims* d, int64_t* off) {
  long o = 0;
  for (int l = 0; l < DCUE_N_BN; ++l) {
    off[2 * l] = o;
    o = al4(o + bn_channels(d, l));
    off[2 * l + 1] = o;
    o = al4(o + bn_channels(d, l));
  }
  off[2 * DCUE_N_BN] = o;
}

}  // namespace

namespace dcue {

int bn_channels(const dcue_dims* d, int l) {
  return l == 0 ? kMels : l == 5 ? st_feature(d) : st_hidden(d);
}

void rebase_acc(Ws* w, unsigned long long* acc) {
  w->bnacc = acc;
  w->rng = reinterpret_cast<unsigned*>(acc + 6L * 2 * w->cmax * 2);
  w->tticket = w->ntick ? reinterpret_cast<unsigned*>(acc + 6L * 2 * w->cmax * 2 + kRngWords) : nullptr;
  w->bnbacc = acc + 6L * 2 * w->cmax * 2 + kRngWords + w->ntick;
  w->grng = reinterpret_cast<unsigned*>(w->bnbacc + 6L * 2 * w->cmax * 2);
}

size_t carve(const dcue_dims* d, int B, int N, int M, void* base, Ws* w) {
  Arena ar{(char*)base, 0, 0};
  const int H = st_hidden(d), D = st_feature(d), E = d->user_embdim;
  const int Cmax = H > kMels ? H : kMels;
  w->counts = ar.take<float>(M);
  w->copy_ptr = ar.take<int32_t>(M + 1);
  w->copy_idx = ar.take<int32_t>((long)B * (N + 1));
  for (int l = 0; l < 6; ++l) {
    const int C = bn_channels(d, l);
    w->mean[l] = ar.take<float>(C);
    w->invstd[l] = ar.take<float>(C);
    w->a[l] = ar.take<float>(C);
    w->bcp[l] = ar.take<float>(C);
  }
  w->cmax = Cmax > D ? Cmax : D;
  // text tower: one 32-bit ticket per (item, column block of >= 64 columns), in 16-B units
  w->ntick = tower_text(d) ? ((long)M * (st_text(d) / 64) + 3) / 4 * 2 : 0;
  w->nfwd = 6L * 2 * w->cmax * 2 + kRngWords + w->ntick;
  w->nzero = w->nfwd + 6L * 2 * w->cmax * 2 + kGrngWords;
  w->bnacc = ar.take<unsigned long long>(w->nzero);
  rebase_acc(w, w->bnacc);
  w->rowsum = ar.take<float>(B);
  w->y[0] = nullptr;
  w->idx[0] = nullptr;
  for (int l = 1; l <= 5; ++l) {
    const long n = (long)M * layer_geom(l).lp * (l == 5 ? D : H);
    w->y[l] = ar.take<float>(n);
    w->idx[l] = ar.take<uint8_t>(n);
  }
  w->f = ar.take<float>((long)M * D);
  w->uf = ar.take<float>((long)B * D);
  w->h1 = ar.take<float>((long)B * E);
  w->cosv = ar.take<float>((long)B * (N + 1));
  w->norms = ar.take<float>((long)B * (N + 2));
  w->hinge = ar.take<float>((long)B * (N > 0 ? N : 1));
  w->scores = ar.take<float>((long)B * (N > 0 ? N : 1));
  w->loss = ar.take<float>(4);
  w->dhinge = ar.take<float>((long)B * (N > 0 ? N : 1));
  w->du = ar.take<float>((long)B * D);
  w->dfcopy = ar.take<float>((long)B * (N + 1) * D);
  w->df = ar.take<float>((long)M * D);
  w->g[0] = nullptr;
  for (int l = 1; l <= 5; ++l) w->g[l] = ar.take<float>((long)M * layer_geom(l).lp * (l == 5 ? D : H));
  w->dh1 = ar.take<float>((long)B * E);
  w->de = ar.take<float>((long)B * E);
  const long nch1 = wgrad_nchunk(1, M, H, kMels, true);  // (so the size never falls as M grows)
  w->wpart = ar.take<float>(nch1 * H * kMels * layer_geom(1).ks);
  w->bpart = ar.take<float>(nch1 * 5 * H);
  for (int l = 2; l <= 6; ++l) {  // 6: the fc layer (a 1x1 conv over bn5(y5), D -> D)
    const int cin = l == 6 ? D : H, cout = l >= 5 ? D : H;
    const long nch = wgrad_nchunk(l, M, cout, cin, true);  // (so the size never falls as M grows)
    w->wpm[l - 2] = ar.take<float>(nch * cout * cin * layer_geom(l == 6 ? 5 : l).ks);
    w->bpm[l - 2] = ar.take<float>(nch * cout);
  }
  w->G = ar.take<float>((long)H * 4 * kMels);
  w->S = ar.take<float>(5L * H);  // the five layer-1 bias partial sums E[5][H]
  w->xhat0 = ar.take<float>((long)(M + 1) * kXp * kMels);  // + a zero item
  w->dx1 = ar.take<float>((long)M * layer_geom(1).lp * H);
  w->ones = w->zeros = w->sink = w->xfc = w->dtp = w->twpart = nullptr;
  w->tidx = nullptr;
  w->tpart = nullptr;
  if (!tower_has_bn(d)) {
    w->ones = ar.take<float>(w->cmax);
    w->zeros = ar.take<float>(w->cmax);
    w->sink = ar.take<float>(2L * w->cmax);
  }
  if (tower_res(d)) {
    w->xfc = ar.take<float>((long)M * fc_in(d));
    w->dtp = ar.take<float>((long)M * 4 * d->conv_hidden);  // the fc input's block columns: reference H
  }
  if (tower_text(d)) {
    const long CT = st_text(d);
    w->xfc = ar.take<float>((long)M * fc_in(d));
    w->dtp = ar.take<float>((long)M * CT);
    w->tidx = ar.take<uint8_t>((long)M * CT);
    w->tpart = ar.take<unsigned long long>((long)M * 2 * CT);
    w->twpart = ar.take<float>((long)text_wgrad_nchunk(M) * (CT * d->word_dim * 3 + CT));
  }
  return ar.used + 256;
}

int step_ws(const dcue_model* m, const dcue_batch* b, void* ws, size_t ws_bytes, const StepOpts& o, Ws* w) {
  if (carve(&m->dims, b->n_rows, b->n_neg, b->n_items, nullptr, w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  carve(&m->dims, b->n_rows, b->n_neg, b->n_items, ws, w);
  if (o.acc) rebase_acc(w, o.acc);
  if (o.counts) w->counts = const_cast<float*>(o.counts);
  if (o.y1) w->y[1] = o.y1;
  return DCUE_OK;
}

long step_acc_words(const dcue_dims* d, int B, int N, int M) {
  Ws w;
  carve(d, B, N, M, nullptr, &w);
  return w.nzero;
}

int init_ctx(Ctx* c, const dcue_model* m) {
  int st = check_dims(&m->dims);
  if (st) return st;
  if (!m->params || !m->bn_stats || !m->bn_batches || !m->wpack) return DCUE_ERR_INVALID;
  // deferred user-table Adam needs its log, the moments it replays and a valid history capacity
  if (m->emb_step && (!m->emb_log || !m->emb || !m->emb_exp_avg || !m->emb_exp_avg_sq ||
                      m->emb_log_cap < 1 || m->emb_log_cap > DCUE_MAX_LOG_CAP))
    return DCUE_ERR_INVALID;
  c->m = m;
  param_offsets(&m->dims, c->poff);
  bn_offsets(&m->dims, c->boff);
  c->H = st_hidden(&m->dims);
  c->D = st_feature(&m->dims);
  c->HL = m->dims.conv_hidden;
  c->E = m->dims.user_embdim;
  c->bn = tower_has_bn(&m->dims);
  c->res = tower_res(&m->dims);
  c->text = tower_text(&m->dims);
  c->FI = fc_in(&m->dims);
  c->off5 = fc_off5(&m->dims);
  c->CT = st_text(&m->dims);
  if (c->text && (!m->words || m->n_words <= 0)) return DCUE_ERR_INVALID;
  return DCUE_OK;
}

int check_batch(const dcue_batch* b) {
  if (!b || !b->users || !b->item_track || b->n_rows <= 0 || b->n_neg < 0 || b->n_items <= 0)
    return DCUE_ERR_INVALID;
  if (b->layout == DCUE_LAYOUT_CATALOGUE) {
    if ((long)b->n_items != (long)b->n_rows * (1 + b->n_neg)) return DCUE_ERR_INVALID;
  } else if (b->layout == DCUE_LAYOUT_GATHER) {
    if (b->n_neg > 0 && !b->neg_item) return DCUE_ERR_INVALID;
    if (b->n_items < b->n_rows) return DCUE_ERR_INVALID;
  } else {
    return DCUE_ERR_INVALID;
  }
  return DCUE_OK;
}

}  // namespace dcue

extern "C" {

int dcue_abi_version(void) { return DCUE_ABI_VERSION; }

int64_t dcue_launch_count(void) { return launches_counted(); }

int dcue_storage_dims(const dcue_dims* dims, dcue_dims* storage_host) {
  TRY(check_dims(dims));
  if (!storage_host) return DCUE_ERR_INVALID;
  *storage_host = *dims;
  storage_host->conv_hidden = st_hidden(dims);
  storage_host->feature_dim = st_feature(dims);
  return DCUE_OK;
}

int dcue_param_layout(const dcue_dims* dims, int64_t* offsets_host) {
  TRY(check_dims(dims));
  if (!offsets_host) return DCUE_ERR_INVALID;
  param_offsets(dims, offsets_host);
  return DCUE_OK;
}

int dcue_bn_layout(const dcue_dims* dims, int64_t* offsets_host) {
  TRY(check_dims(dims));
  if (!offsets_host) return DCUE_ERR_INVALID;
  bn_offsets(dims, offsets_host);
  return DCUE_OK;
}

int dcue_wpack_floats(const dcue_dims* dims, int64_t* n) {
  TRY(check_dims(dims));
  if (!n) return DCUE_ERR_INVALID;
  *n = wpack_layout(dims).total;
  return DCUE_OK;
}

int dcue_workspace_bytes(const dcue_dims* dims, int32_t max_rows, int32_t max_neg,
                         int32_t max_items, size_t* bytes) {
  TRY(check_dims(dims));
  if (!bytes || max_rows <= 0 || max_neg < 0 || max_items <= 0) return DCUE_ERR_INVALID;
  Ws w;
  *bytes = carve(dims, max_rows, max_neg, max_items, nullptr, &w);
  return DCUE_OK;
}

int dcue_debug_launch_shape(const dcue_dims* dims, int32_t layout, int32_t B, int32_t N, int32_t M,
                            int32_t* out_host, int32_t cap) {
  TRY(check_dims(dims));
  if (!out_host || cap < DCUE_LAUNCH_SHAPE_WORDS || B <= 0 || N < 0 || M <= 0) return DCUE_ERR_INVALID;
  const bool gather = layout == DCUE_LAYOUT_GATHER;
  if (layout == DCUE_LAYOUT_CATALOGUE ? (long)M != (long)B * (1 + N) : (!gather || M < B)) return DCUE_ERR_INVALID;
  // the arguments backward_impl / forward_impl give the launchers (step_backward.hip, step_forward.hip)
  const int H = st_hidden(dims), D = st_feature(dims);
  const bool fc = !tower_res(dims) && !tower_text(dims);  // the fc rides in the item gradient / layer 3-5 launch
  int32_t* o = out_host;
  for (int l = 1; l <= 5; ++l, o += 5) conv_fwd_shape(l, l == 1 ? kMels : H, l == 5 ? D : H, M, o);
  for (int l = 2; l <= 5; ++l, o += 5) conv_dgrad_shape(l, l == 5 ? D : H, H, M, o);
  for (int l = 1; l <= 6; ++l, o += 4) {
    if (l == 6 && !fc) {  // res / text towers: the fc weight gradient is a plain GEMM
      o[0] = -1;
      o[1] = o[2] = o[3] = 0;
      continue;
    }
    wgrad_shape(l, M, l >= 5 ? D : H, l == 1 ? kMels : l == 6 ? D : H, l <= 2, o);
  }
  tail_shape(N, M, D, gather, gather && M <= kCopyListMaxItems, fc, o);
  return DCUE_OK;
}

int dcue_debug_text_shape(const dcue_dims* dims, int32_t M, int32_t* out_host, int32_t cap) {
  TRY(check_dims(dims));
  if (!tower_text(dims) || !out_host || cap < DCUE_TEXT_SHAPE_WORDS || M <= 0) return DCUE_ERR_INVALID;
  // the arguments text_branch gives the launchers, the knobs at their defaults
  const TextFwdShape f = text_fwd_shape(M, dims->text_len, st_word(dims), st_text(dims), false, 81, 1, true, 6);
  if (!f.valid) return DCUE_ERR_INVALID;
  const TextWgradShape g = text_wgrad_shape(M);
  int32_t* o = out_host;
  o[0] = f.full ? 0 : 1;
  o[1] = f.tb; o[2] = f.wv; o[3] = f.nct; o[4] = f.full ? f.bpd : 0; o[5] = f.nch;
  o[6] = f.full ? f.nxcd : 0;
  o[7] = (int32_t)f.nunit; o[8] = (int32_t)f.grid;
  o[9] = (int32_t)f.lds; o[10] = (int32_t)f.lds_static; o[11] = f.last;
  o[12] = g.nchunk; o[13] = g.items_per_chunk; o[14] = g.last; o[15] = g.reduce ? 1 : 0;
  return DCUE_OK;
}

int dcue_workspace_outputs(const dcue_dims* dims, int32_t B, int32_t N, int32_t M,
                           size_t* offsets_host) {
  TRY(check_dims(dims));
  if (!offsets_host || B <= 0 || N < 0 || M <= 0) return DCUE_ERR_INVALID;
  Ws w;
  carve(dims, B, N, M, nullptr, &w);
  offsets_host[0] = (size_t)w.scores;
  offsets_host[1] = (size_t)w.uf;
  offsets_host[2] = (size_t)w.f;
  offsets_host[3] = (size_t)w.loss;
  return DCUE_OK;
}

int dcue_workspace_activations(const dcue_dims* dims, int32_t B, int32_t N, int32_t M,
                               size_t* offsets_host) {
  TRY(check_dims(dims));
  if (!offsets_host || B <= 0 || N < 0 || M <= 0) return DCUE_ERR_INVALID;
  Ws w;
  carve(dims, B, N, M, nullptr, &w);
  for (int l = 1; l <= 5; ++l) {
    offsets_host[2 * (l - 1)] = (size_t)w.y[l];
    offsets_host[2 * (l - 1) + 1] = (size_t)w.idx[l];
  }
  return DCUE_OK;
}

int dcue_workspace_text(const dcue_dims* dims, int32_t B, int32_t N, int32_t M, size_t* offsets_host) {
  TRY(check_dims(dims));
  if (!tower_text(dims) || !offsets_host || B <= 0 || N < 0 || M <= 0) return DCUE_ERR_INVALID;
  Ws w;
  carve(dims, B, N, M, nullptr, &w);
  offsets_host[0] = (size_t)w.xfc;
  offsets_host[1] = (size_t)w.dtp;
  offsets_host[2] = (size_t)w.tidx;
  return DCUE_OK;
}

int dcue_pack_weights(const dcue_model* m, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  TRY(join_user_stream((hipStream_t)stream));
  return launch_pack(m, c.poff, (hipStream_t)stream);
}

int dcue_forward(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws,
                 size_t ws_bytes, int32_t train, float margin, float* scores, float* user_feat,
                 float* item_feat, float* loss, void* stream) {
  // a plan step may leave Adam work on the user stream (its late dense segments, the user table)
  TRY(join_user_stream((hipStream_t)stream));
  TRY(dcue::forward_impl(m, b, t, ws, ws_bytes, train, margin, StepOpts{}, (hipStream_t)stream));
  // the outputs live in the workspace (dcue_workspace_outputs gives their offsets); copies are
  // made only for callers that ask for their own buffers
  Ws w;
  carve(&m->dims, b->n_rows, b->n_neg, b->n_items, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  const int B = b->n_rows, N = b->n_neg, M = b->n_items, D = st_feature(&m->dims);
  if (scores && N > 0) DCUE_HIP_CHECK(hipMemcpyAsync(scores, w.scores, sizeof(float) * B * N, hipMemcpyDeviceToDevice, s));
  if (user_feat) DCUE_HIP_CHECK(hipMemcpyAsync(user_feat, w.uf, sizeof(float) * B * D, hipMemcpyDeviceToDevice, s));
  if (item_feat) DCUE_HIP_CHECK(hipMemcpyAsync(item_feat, w.f, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, s));
  if (loss) DCUE_HIP_CHECK(hipMemcpyAsync(loss, w.loss, sizeof(float), hipMemcpyDeviceToDevice, s));
  return DCUE_OK;
}

int dcue_train_backward(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws,
                        size_t ws_bytes, const float* dscores, float emb_grad_scale, void* stream) {
  TRY(join_user_stream((hipStream_t)stream));
  return dcue::backward_impl(m, b, t, ws, ws_bytes, dscores, emb_grad_scale, StepOpts{},
                             (hipStream_t)stream);
}

int dcue_dcbr_step(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, const float* target,
                   float* loss, void* ws, size_t ws_bytes, void* stream) {
  // the item tower's train forward, the MSE head and the item tower's backward (dcue.h)
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!b || !t || !t->data || !target || !ws || !m->grads || !b->item_track) return DCUE_ERR_INVALID;
  if (b->layout != DCUE_LAYOUT_CATALOGUE || b->n_neg != 0 || b->n_rows <= 0 || b->n_items != b->n_rows)
    return DCUE_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  TRY(join_user_stream(s));
  Ws w;
  const int M = b->n_items;
  TRY(step_ws(m, b, ws, ws_bytes, StepOpts{}, &w));
  TRY(launch_item_counts(b, w.counts, s));
  TRY(item_forward(c, w, t, b->item_track, M, (double)M, true, w.counts, nullptr, s));
  TRY(launch_mse_grad(w.f, target, M, m->dims.feature_dim, c.D, w.dfcopy, w.rowsum, w.loss, s));
  if (loss) DCUE_HIP_CHECK(hipMemcpyAsync(loss, w.loss, sizeof(float), hipMemcpyDeviceToDevice, s));
  StepOpts o;
  o.item_only = true;
  return dcue::backward_impl(m, b, t, ws, ws_bytes, nullptr, 1.f, o, s);
}

int dcue_adam_step(const dcue_model* m, const dcue_adam_args* a, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!a || a->step < 1 || (a->parts & ~(DCUE_ADAM_DENSE | DCUE_ADAM_EMBEDDING))) return DCUE_ERR_INVALID;
  const int parts = a->parts ? a->parts : (DCUE_ADAM_DENSE | DCUE_ADAM_EMBEDDING);
  if ((parts & DCUE_ADAM_DENSE) && (!m->grads || !m->exp_avg || !m->exp_avg_sq)) return DCUE_ERR_INVALID;
  if ((parts & DCUE_ADAM_EMBEDDING) &&
      (!m->emb || !m->emb_exp_avg || !m->emb_exp_avg_sq || !m->emb_slot || !m->emb_grad))
    return DCUE_ERR_INVALID;
  if ((parts & DCUE_ADAM_EMBEDDING) && m->emb_step && !m->emb_rows) return DCUE_ERR_INVALID;
  TRY(join_user_stream((hipStream_t)stream));
  TRY(launch_adam(m, a, c.poff, (hipStream_t)stream));
  // the dense sweep repacked the conv weights as it went (k_adam_dense_pack)
  return DCUE_OK;
}

int dcue_optimizer_step(const dcue_model* m, const dcue_opt_args* a, const dcue_opt_state* st, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!a || !st || a->step < 1 || !m->grads || !m->emb || !m->emb_slot) return DCUE_ERR_INVALID;
  if (m->dims.n_users > 0 && !m->emb_grad) return DCUE_ERR_INVALID;
  if (a->kind == DCUE_OPT_SGD) {
    if (!st->dense_a || !st->emb_a) return DCUE_ERR_INVALID;
  } else if (a->kind == DCUE_OPT_RANGER) {
    if (!st->dense_a || !st->dense_b || !st->dense_c || !st->emb_a || !st->emb_b || !st->emb_c || a->k < 1)
      return DCUE_ERR_INVALID;
  } else {
    return DCUE_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  TRY(join_user_stream(s));
  TRY(launch_opt(m, a, st, c.poff[kSeg], s));
  return launch_pack(m, c.poff, s);
}

int dcue_item_tower_eval(const dcue_model* m, const dcue_tracks* t, const int32_t* item_track,
                         int32_t n_items, void* ws, size_t ws_bytes, float* item_feat,
                         void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!t || !t->data || !item_track || !ws || !item_feat || n_items <= 0) return DCUE_ERR_INVALID;
  Ws w;
  if (carve(&m->dims, 1, 0, n_items, nullptr, &w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  carve(&m->dims, 1, 0, n_items, ws, &w);
  TRY(join_user_stream((hipStream_t)stream));
  return item_forward(c, w, t, item_track, n_items, (double)n_items, false, nullptr, item_feat,
                      (hipStream_t)stream);
}

int dcue_user_tower(const dcue_model* m, const int64_t* users, int32_t n, void* ws, size_t ws_bytes,
                    float* user_feat, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!users || !ws || !user_feat || n <= 0 || !m->emb) return DCUE_ERR_INVALID;
  Ws w;
  if (carve(&m->dims, n, 0, 1, nullptr, &w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  carve(&m->dims, n, 0, 1, ws, &w);
  TRY(join_user_stream((hipStream_t)stream));
  if (m->emb_step) TRY(launch_emb_sync(m, users, n, (hipStream_t)stream));
  return user_forward(c, w, users, n, user_feat, (hipStream_t)stream);
}

int dcue_emb_log_bytes(int32_t cap, size_t* bytes_host) {
  if (!bytes_host || cap < 1 || cap > DCUE_MAX_LOG_CAP) return DCUE_ERR_INVALID;
  *bytes_host = sizeof(dcue_emb_log) + (size_t)cap * 8 * sizeof(float);
  return DCUE_OK;
}

int dcue_emb_log_init(const dcue_model* m, int32_t cap, int32_t step, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!m->emb_step || !m->emb_log || cap < 1 || cap > DCUE_MAX_LOG_CAP || cap != m->emb_log_cap ||
      step < 0)
    return DCUE_ERR_INVALID;
  TRY(join_user_stream((hipStream_t)stream));
  return launch_emb_log_init(m, cap, step, (hipStream_t)stream);
}

int dcue_embedding_sync(const dcue_model* m, const int64_t* users, int32_t n, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!users || n < 0) return DCUE_ERR_INVALID;
  if (!m->emb_step) return DCUE_OK;  // dense mode: rows are always current
  TRY(join_user_stream((hipStream_t)stream));
  return launch_emb_sync(m, users, n, (hipStream_t)stream);
}

int dcue_embedding_flush(const dcue_model* m, void* stream) {
  Ctx c;
  TRY(init_ctx(&c, m));
  if (!m->emb_step) return DCUE_OK;
  TRY(join_user_stream((hipStream_t)stream));
  return launch_emb_flush(m, (hipStream_t)stream);
}

}  // extern "C"
