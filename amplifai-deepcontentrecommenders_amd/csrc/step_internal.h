// Shared by the step units (step_forward.hip, step_backward.hip) and capi.hip, which defines the layouts:
// the workspace's carved pointers, the per-call model context, the layer / segment helpers.
#pragma once

#include "dcue_internal.h"

namespace dcue {

constexpr int kSeg = DCUE_N_DENSE_SEGMENTS;

// pointers into the caller's workspace
struct Ws {
  float* counts;
  int32_t *copy_ptr, *copy_idx;  // gather layout: per-item copy lists (StepPrologue), M <= kCopyListMaxItems
  float *mean[6], *invstd[6], *a[6];
  float* bcp[6];  // the step's BN betas as the forward used them (BnPublish::beta_out)
  // exact BN sums (bnacc.h), [6 layers][2 sums][Cmax][2 words]: forward stats, backward sums
  unsigned long long *bnacc, *bnbacc;
  // the forward's value ranges (split-f16 operand scales, conv_rows.h / conv_wgrad.hip): [6 layers]
  // [2][kRngC] ordered keys, between the forward and backward sums of the block (cleared with the
  // forward sums); the backward's gradient maxima [7][kRngC] (max |g_l| for l = 1..5, max |df| at 6)
  // after the backward sums (cleared with them)
  unsigned* rng;
  unsigned* grng;
  long nzero;            // words of the accumulator block (one clear per step)
  long nfwd;             // its forward part: the sums and the ranges
  float* rowsum;         // [B] per-row hinge sums (score_fused)
  int cmax;
  float* y[6];
  uint8_t* idx[6];
  float *f, *uf, *h1;
  float *cosv, *norms, *hinge, *scores, *loss, *dhinge;
  float *du, *dfcopy, *df;
  float* g[6];
  float *dh1, *de;
  float *wpart, *bpart, *G, *S;  // the conv-1 weight gradient's split-K partials, its reduce's outputs
  float *wpm[5], *bpm[5];                // k_conv_wgrad_multi's partials, layers 2..5 and the fc
  float* xhat0;          // [M][kXp][128] bn0-normalised, zero-padded input: conv-1 wgrad's X operand
  float* dx1;            // [M][33][H] BN1 backward at the pooled positions: conv-1 wgrad's dz operand
  // towers without BN: the BN operands every kernel reads become the identity (mean 0, a = invstd
  // = 1, beta 0) and the BN parameter gradients go to a scratch sink
  float *ones, *zeros, *sink;
  // res towers: the fc input [M][4H + d] (time-pooled blocks 1-4, then block 5) and the gradient
  // of the four time-pooled outputs [M][4H]; text tower: the fc input [M][text_dim + d] (text
  // features, then block 5) and the text features' gradient [M][C_s]
  float *xfc, *dtp;
  uint8_t* tidx;  // text tower: [M][C_s] the max-over-positions argmax (255: no gradient)
  // text tower: the forward's position-part merge (TextBranch::ticket / part): tickets in the
  // accumulator block's forward part (ntick 64-bit words, cleared with it), maxima [M][2][C_s]
  unsigned* tticket;
  unsigned long long* tpart;
  long ntick;
  float* twpart;  // text tower: the text conv's weight-gradient chunk partials
};

// the accumulator block's parts: [6][2][Cmax][2] forward sums, then the same for the backward
constexpr long kRngWords = 6L * 2 * kRngC / 2;   // the ranges' 64-bit words
constexpr long kGrngWords = 7L * kRngC / 2 + 64;  // the gradient maxima's (+ padding to keep 16-B alignment)

void rebase_acc(Ws* w, unsigned long long* acc);
// carves B x N x M's workspace at `base` (null: sizes only); returns the bytes it needs
size_t carve(const dcue_dims* d, int B, int N, int M, void* base, Ws* w);
// a step's workspace: checked against ws_bytes, carved, then the plan's own accumulator block, copy
// counts and conv-1 output (StepOpts::acc / counts / y1) in place of the workspace's
int step_ws(const dcue_model* m, const dcue_batch* b, void* ws, size_t ws_bytes, const StepOpts& o, Ws* w);

// layer l's range (l = 0: the raw input of conv 1; l = 1..5: the ReLU output of conv l)
inline unsigned* rng_at(const Ws& w, int l) { return w.rng + (size_t)l * 2 * kRngC; }
// max |g_l| per channel (l = 1..5), max |df| (l = 6)
inline unsigned* grng_at(const Ws& w, int l) { return w.grng + (size_t)l * kRngC; }
inline unsigned long long* bn_acc(unsigned long long* base, int cmax, int l) {
  return base + (size_t)l * 2 * cmax * 2;
}
int bn_channels(const dcue_dims* d, int l);

struct Ctx {
  const dcue_model* m;
  int64_t poff[kSeg + 1];
  int64_t boff[2 * DCUE_N_BN + 1];
  int H, D, E;   // storage widths (H, d padded to 32/64/128/256) and E
  int HL;        // the reference's conv_hidden: column width of the res towers' time-pooled blocks
  bool bn, res;  // tower variant (dcue_dims.tower)
  bool text;     // the mixed audio + text tower (text.hip)
  int FI;        // fc input width: D, 4H + D in the res towers, text_dim + D in the text tower
  int off5;      // first fc-input column of bn5(y5)
  int CT;        // text tower: storage channels of the text branch
  const float* P(int seg) const { return m->params + poff[seg]; }
  float* Gd(int seg) const { return m->grads + poff[seg]; }
  float* rmean(int l) const { return m->bn_stats + boff[2 * l]; }
  float* rvar(int l) const { return m->bn_stats + boff[2 * l + 1]; }
  // BN_l's gamma / beta as the kernels read them, and where their gradients go; the identity and a
  // scratch sink in the towers without BN
  const float* gamma(const Ws& w, int l) const { return bn ? P(seg_bn_w(l)) : w.ones; }
  const float* beta(const Ws& w, int l) const { return bn ? P(seg_bn_b(l)) : w.zeros; }
  // the backward's view of BN l's beta: the forward's snapshot (the parameter itself may already be
  // stepping: split plans run Adam over bn1 beside the layer-2 weight gradient that reads it)
  const float* beta_bwd(const Ws& w, int l) const { return bn ? w.bcp[l] : w.zeros; }
  float* dgamma(const Ws& w, int l) const { return bn ? Gd(seg_bn_w(l)) : w.sink; }
  float* dbeta(const Ws& w, int l) const { return bn ? Gd(seg_bn_b(l)) : w.sink + w.cmax; }
};
int init_ctx(Ctx* c, const dcue_model* m);

int check_batch(const dcue_batch* b);
// whether a gather batch gets per-item copy lists (the prologue's histogram path)
inline bool copy_lists(const dcue_batch* b) {
  return b->layout == DCUE_LAYOUT_GATHER && b->n_items <= kCopyListMaxItems;
}
inline int track_src(const dcue_tracks* t) { return t->dtype == 0 ? SRC_TRACK_F16 : SRC_TRACK_F32; }
// C[m][n] (rows scm apart) = sum_k A[m * sam + k * sak] B[k * sbk + n * sbn]: launch_tgemm's plain operands
inline TGemmArgs gemm_args(int M, int N, int K, const float* A, long sam, long sak, const float* B, long sbk,
                           long sbn, float* C, long scm) {
  TGemmArgs g = {};
  g.M = M; g.N = N; g.K = K;
  g.A = A; g.sam = sam; g.sak = sak;
  g.B = B; g.sbk = sbk; g.sbn = sbn;
  g.C = C; g.scm = scm; g.scn = 1;
  return g;
}
// the text branch's operands (text tower); t->tokens must be set
TextBranch text_branch(const Ctx& c, const dcue_tracks* t);

// ----------------------------------------------------------------- the towers (step_forward.hip)
// item_forward's options beyond the plain tower (eval, DCBR: all defaults)
struct ItemFwdOpts {
  bool acc_cleared = false;  // the forward sums and ranges start cleared (the step prologue did it)
  bool stats_done = false;   // bn0's batch sums are already in the accumulator block (plans, lookahead)
  bool clear_bn0 = false;    // ... of a batch announced ahead but not the one launched: cleared first
  Edge before_l2;            // split plans: the previous step's late Adam, which conv 2 follows
  dcue_comm* sync_bn = nullptr;
  unsigned* start_sig = nullptr;  // plans: conv 1 raises the step's start signal
  // called with `hook` right after conv 1 / in place of the text branch's launch (forward_impl's user
  // part and text join); null: nothing / the text branch on the caller's stream
  int (*after_l1)(void*) = nullptr;
  int (*text_join)(void*) = nullptr;
  void* hook = nullptr;
};
// Item tower forward. train: batch statistics (weighted by counts, accumulated exactly by the
// producing kernels) + running-stat update by each BN's first consumer; eval: running statistics.
int item_forward(const Ctx& c, const Ws& w, const dcue_tracks* t, const int32_t* item_track, int M,
                 double copies, bool train, const float* counts, float* f_out, hipStream_t s,
                 const ItemFwdOpts& io = ItemFwdOpts{});
// user tower (userembedding.py:33-44): h1 = relu(E[u]) W1^T + b1; uf = relu(h1) W2^T + b2, as two
// k_tgemm launches (eval; DCUE_USER_FWD=split)
int user_forward(const Ctx& c, const Ws& w, const int64_t* users, int B, float* uf_out, hipStream_t s);

}  // namespace dcue
