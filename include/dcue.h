/*
 * dcue.h -- C ABI of libdcue_hip.so, the MI355X (gfx950) DCUE training-step library.
 *
 * The reference (estebandito22/Amplifai-DeepContentRecommenders) is pure Python/PyTorch; its
 * "operator interface" for the hot path is the torch module/trainer API listed per entry point
 * below. These entry points are what a ctypes binding of that interface calls.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless the name ends in _host. The caller (PyTorch's caching
 *    allocator in the shipped binding) owns every buffer; the library allocates nothing.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*) and returns a
 *    dcue_status; argument errors are detected on the host before anything is launched.
 *  - Float math is fp32 throughout (f32-input MFMA, exact f32 products); spectrogram tables may be
 *    stored as fp16 (lossless for fp16-representable inputs) or fp32.
 *  - Layouts: spectrogram table [n_tracks][n_frames=131][n_mels=128] (frame-major rows of mel bins);
 *    dense parameters are ONE flat fp32 buffer in reference parameter order and reference tensor
 *    layouts (offsets from dcue_param_layout); the user-embedding table is a separate
 *    [n_users][user_embdim] buffer (sharded by user across ranks).
 */
#ifndef DCUE_H_
#define DCUE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCUE_ABI_VERSION 17
#define DCUE_N_MELS 128
#define DCUE_N_FRAMES 131
#define DCUE_N_BN 6
/* dense parameter segments, reference order (DCUENet.named_parameters(), minus the embeddings):
 * 28 of the reference's DCUENet, then the text tower's text.conv.{weight, bias} (empty in the
 * audio-only towers) */
#define DCUE_N_DENSE_SEGMENTS 30

typedef enum {
  DCUE_OK = 0,
  DCUE_ERR_INVALID = 1,     /* bad argument (null pointer, size out of range) */
  DCUE_ERR_UNSUPPORTED = 2, /* valid for the reference, not for this build (e.g. d > 256) */
  DCUE_ERR_HIP = 3,         /* a HIP launch failed */
  DCUE_ERR_WORKSPACE = 4    /* workspace too small */
} dcue_status;

/* Item towers DCUENet wires by model_type (dcue/dcue.py:49-59):
 *   BN    truedcuemel1dbn    bn0 -> 4x[conv, pool, relu, bn] -> conv, relu, bn -> fc(d -> d) (default)
 *   PLAIN truedcuemel1d      the same without any BatchNorm
 *   RES   truedcuemel1dres   no BN; each block's output also time-averaged (AvgPool1d over all its
 *                            positions) and concatenated with the last block: fc(4H + d -> d)
 *   RESBN truedcuemel1dresbn RES with the BN tower's BatchNorms (the averages taken after each BN)
 * In the towers without BN the segments of the BN parameters are empty (dcue_param_layout).
 *   TEXT  BASELINE config 4, the mixed audio + text item encoder (no reference code: the reference's
 *         text item set, datasets/dcuelmitemset.py:8, imports a WordEmbeddings module it never
 *         published; this build's encoder): the BN tower's audio stack plus a text
 *         branch over each track's sentence of token ids (BOS + sentence + EOS, PAD-padded to
 *         text_len, dcuelmitemset.py:40-56): frozen word vectors [n_words][word_dim] (the
 *         LM-pretrained part, caller supplied: dcue_model.words), Conv1d(word_dim -> text_dim, k 3,
 *         pad 1), max over the non-PAD positions, ReLU; f = fc([s ; bn5(y5)]) with fc(text_dim + d -> d).
 *         The text positions' token ids come from dcue_tracks.tokens. */
#define DCUE_TOWER_BN 0
#define DCUE_TOWER_PLAIN 1
#define DCUE_TOWER_RES 2
#define DCUE_TOWER_RESBN 3
#define DCUE_TOWER_TEXT 4

typedef struct dcue_dims {
  int32_t conv_hidden; /* H: nn/dcue.py:45 conv_hidden (1..256; stored padded, dcue_storage_dims) */
  int32_t feature_dim; /* d: feature_dim (1..256; the trainer's default is 100, nn/dcue.py:44) */
  int32_t user_embdim; /* E: u_embdim (<= 1024) */
  int32_t tower;       /* DCUE_TOWER_* */
  int64_t n_users;     /* rows of the (local shard of the) user table */
  /* DCUE_TOWER_TEXT only (0 otherwise): */
  int32_t text_dim;    /* C: text features (1..256; stored at 64/128/256 channels) */
  int32_t word_dim;    /* E_w: word-vector width (4..1024, a multiple of 4) */
  int32_t text_len;    /* T: token positions per track (max_sentence_length + 1; 2..128) */
  int32_t text_pad;    /* PAD token id: positions holding it are left out of the max */
} dcue_dims;

/* Deferred user-table Adam (optional, selected by dcue_model.emb_step != NULL).
 * The reference's dense embedding gradient makes torch.optim.Adam step EVERY user row each batch,
 * with g = 0 (+ wd*p) for rows outside the batch (nn/dcue.py:143-147,209). Deferred mode performs
 * exactly those steps, later: a row's zero-gradient steps are replayed with the same fp32
 * operations and the same per-step scalars (kept in this log's history ring) right before the row
 * is next read (dcue_forward / dcue_user_tower bring their users' rows current), for a rolling
 * 1/cap slice of the table every step (so every row at least once per `cap` steps), and for all
 * rows on dcue_embedding_flush. After a flush the table and both moments are
 * bit-identical to the dense sweep's; between flushes rows outside recent batches lag behind, so
 * read the table directly only after a flush. The [cap][8] float history follows this header. */
typedef struct dcue_emb_log {
  int32_t step_done;   /* last Adam step recorded */
  int32_t flush_step;  /* every row is current to at least this step */
  int32_t n_touched;   /* emb_rows entries written by the last backward */
  int32_t grad_step;   /* the Adam step the last backward's compact gradient belongs to */
  int32_t cap;         /* history ring capacity in steps (= flush period) */
  /* frozen rows (ABI 16): the epoch whose steps all keep long-idle rows long idle -- its first step
   * (0: none), the largest |lr / bias_correction1| and the smallest eps it admits; a row's clock
   * (emb_step) with bit 30 set is frozen under it. Written by the library only. */
  int32_t frz_start;
  float frz_S;
  float frz_eps;
} dcue_emb_log;

/* Model state. Replaces DCUENet's parameters/buffers (dcue/dcue.py:21-68) + torch.optim.Adam state. */
typedef struct dcue_model {
  dcue_dims dims;
  float* params;       /* flat dense params, dcue_param_layout offsets */
  float* grads;        /* same layout */
  float* exp_avg;      /* Adam first moment, same layout */
  float* exp_avg_sq;   /* Adam second moment, same layout */
  float* emb;          /* [n_users][E] user_embd.embeddings.weight */
  float* emb_exp_avg;
  float* emb_exp_avg_sq;
  float* emb_grad;     /* [max_rows][E] compact rows of the embedding gradient (one per distinct user) */
  int32_t* emb_slot;   /* [n_users] slot of each user row in emb_grad, -1 = no gradient this step */
  float* bn_stats;     /* running_mean/var per BN layer, dcue_bn_layout offsets */
  int64_t* bn_batches; /* [6] num_batches_tracked */
  float* wpack;        /* packed conv weights (dcue_wpack_floats), refreshed by dcue_pack_weights */
  int64_t* emb_rows;   /* [max_rows] user row of each compact gradient row (-1: duplicate user) */
  int32_t* emb_step;   /* deferred mode: [n_users] step each row is current to (NULL: dense sweep) */
  dcue_emb_log* emb_log; /* deferred mode: header + history (dcue_emb_log_bytes) */
  int32_t emb_log_cap;   /* deferred mode: the log's history capacity (1..DCUE_MAX_LOG_CAP) */
  int32_t reserved;
  /* DCUE_TOWER_TEXT: the frozen word vectors text.embeddings.weight [n_words][word_dim] (never
   * updated by the library) and the power of two 2^words_exp the kernels scale them by before their
   * fp16 hi/lo split (exact; choose it so max |word value| * 2^words_exp lies in [2^13, 2^15)) */
  const float* words;
  int64_t n_words;
  int32_t words_exp;
  int32_t reserved2;
} dcue_model;

#define DCUE_MAX_LOG_CAP 256

/* One training batch, already resident in HBM.
 * Items are the spectrograms the item tower runs on. Catalogue mode (datasets/dcuedataset.py:242-250):
 * M = B*(1+N) items, item b = positive of row b, item B+b*N+j = negative j of row b. In-batch mode
 * (nn/dcue.py:698-709): M = B, negative (b,j) is a copy of positive neg_item[b][j]; the library runs
 * the tower once per distinct item and weights BatchNorm statistics by each item's copy count, which
 * is exactly the reference's computation on the duplicated [pos; neg] stack. */
#define DCUE_LAYOUT_CATALOGUE 0 /* M = B*(1+N), item b = positive b, item B+b*N+j = negative (b,j) */
#define DCUE_LAYOUT_GATHER 1    /* positives are items 0..B-1, negative (b,j) = item neg_item[b][j] */

typedef struct dcue_batch {
  int32_t n_rows;            /* B */
  int32_t n_neg;             /* N */
  int32_t n_items;           /* M */
  int32_t layout;            /* DCUE_LAYOUT_* */
  const int64_t* users;      /* [B] local user rows */
  const int32_t* item_track; /* [M] track row of each item */
  const int32_t* neg_item;   /* [B][N] item of each negative copy (GATHER layout; ignored otherwise) */
} dcue_batch;

typedef struct dcue_tracks {
  const void* data;  /* [n_tracks][131][128] */
  int64_t n_tracks;
  int32_t dtype;     /* 0 = fp16, 1 = fp32 */
  int32_t reserved;
  const int32_t* tokens;  /* DCUE_TOWER_TEXT: [n_tracks][text_len] token ids (< n_words) */
} dcue_tracks;

#define DCUE_ADAM_DENSE 1     /* flat dense params, then the conv-weight repack */
#define DCUE_ADAM_EMBEDDING 2 /* the user table */

typedef struct dcue_adam_args {
  /* param_group values set by CyclicLRWithRestarts, as the Python floats torch.optim.Adam reads
   * (double: 1 - beta1 etc. are formed in double and rounded once, as torch does) */
  double lr, beta1, beta2, eps, weight_decay;
  int32_t step;                              /* Adam step count AFTER increment (1 on first step) */
  int32_t parts;                             /* DCUE_ADAM_* mask; 0 = both */
  double grad_div; /* > 1: the dense gradient is first divided by it in place (DDP's mean over
                      grad_div ranks of an all-reduced sum); 0 or 1: used as is */
} dcue_adam_args;

/* ---------------------------------------------------------------------------------- layout */
int dcue_abi_version(void);
/* The HIP call behind the most recent DCUE_ERR_HIP (file:line, call, HIP error), "" if none. */
const char* dcue_last_error(void);
/* Kernel launches the library has issued in this process (all threads and streams; a step replay
 * through a captured graph counts none). Diagnostic: bench.py reports launches per step from it. */
int64_t dcue_launch_count(void);
/* Storage widths. Any conv_hidden / feature_dim in 1..256 is accepted (DCUENet takes any,
 * dcue/dcue.py:39-47). The library stores and computes them at the width rounded up to 32, 64, 128
 * or 256: every dense segment below is laid out for the storage dims (e.g. conv.layer5.weight is
 * [d_s][H_s][1], conv.fc.weight [d_s][d_s], or [d_s][4H + d_s] in the res towers, whose four
 * time-pooled blocks keep H columns each), and the reference-shaped parameter is the leading
 * [:d, :H, ...] corner of its segment. The caller zero-fills everything outside those corners
 * (weights, biases, BN gamma/beta and running statistics); the padded channels then carry exact
 * zeros through forward, backward and every optimizer, so they never leave zero and the corners
 * compute the reference model. Item / user feature outputs are [.][d_s] rows, zero past d. */
int dcue_storage_dims(const dcue_dims* dims, dcue_dims* storage_host);
/* offsets[DCUE_N_DENSE_SEGMENTS+1] (floats) of each dense parameter in `params` (storage dims) */
int dcue_param_layout(const dcue_dims* dims, int64_t* offsets_host);
/* offsets[2*DCUE_N_BN+1]: running_mean(l), running_var(l) for l = 0..5 */
int dcue_bn_layout(const dcue_dims* dims, int64_t* offsets_host);
int dcue_wpack_floats(const dcue_dims* dims, int64_t* n_floats_host);
/* Bytes of a workspace for batches of up to max_rows rows, max_neg negatives and max_items items: never
 * smaller than for any smaller batch, so one sized for the largest batch serves every smaller one. */
int dcue_workspace_bytes(const dcue_dims* dims, int32_t max_rows, int32_t max_neg,
                         int32_t max_items, size_t* bytes_host);
/* Byte offsets inside a workspace carved for (B, N, M) of the forward outputs a train/eval
 * dcue_forward leaves there: [0] scores [B][N], [1] user feats [B][d_s], [2] item feats [M][d_s],
 * [3] loss (one float). Valid until the next call on the same workspace. */
int dcue_workspace_outputs(const dcue_dims* dims, int32_t B, int32_t N, int32_t M,
                           size_t* offsets_host);
/* Inspection (tests): byte offsets of the train forward's per-layer activations in the same
 * workspace. offsets[2(l-1)] = y_l, float [M][Lp_l][C_l] = relu(max-pooled conv + bias), before
 * BN; offsets[2(l-1)+1] = its uint8 [M][Lp_l][C_l] window argmax (0..pool-1, first maximum), for
 * conv layers l = 1..5 (Lp = 33, 8, 2, 1, 1; C = H_s, H_s, H_s, H_s, d_s: storage widths). */
int dcue_workspace_activations(const dcue_dims* dims, int32_t B, int32_t N, int32_t M,
                               size_t* offsets_host);
/* Inspection (tests; added under ABI 17): byte offsets of the text branch's slices in the same
 * workspace after a train step. [0] xfc, float [M][text_dim + d_s]: the fc input, the text features
 * s in columns [0, text_dim), then bn5(y5); [1] dtp, float [M][C_s]: dL/ds, the text features'
 * gradient before the ReLU / max routing; [2] tidx, uint8 [M][C_s]: the position of the maximum over
 * the non-PAD positions (first maximum), 255 = no gradient (maximum <= 0, no valid position, or a
 * storage channel >= text_dim). C_s = text_dim rounded up to 64, 128 or 256. DCUE_ERR_INVALID
 * outside the text tower. */
int dcue_workspace_text(const dcue_dims* dims, int32_t B, int32_t N, int32_t M, size_t* offsets_host);

/* ------------------------------------------------------------------------- hot-path entries */
/* Refresh wpack from params (after any host-side write of conv weights and after every Adam step). */
int dcue_pack_weights(const dcue_model* m, void* stream);

/* Forward: DCUENet.forward(u, pos, neg) (dcue/dcue.py:70-108) + hinge loss (nn/dcue.py:167-170).
 * train != 0: model.train() semantics -- BatchNorm batch statistics over all copies, running stats
 * and num_batches_tracked updated, activations kept in `ws` for dcue_train_backward.
 * train == 0: model.eval() semantics (running statistics, nothing updated).
 * Outputs (each nullable): scores[B][N], user feats [B][d_s], item feats [M][d_s], loss[1] (mean over
 * rows of the summed hinge). */
int dcue_forward(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws,
                 size_t ws_bytes, int32_t train, float margin, float* scores, float* user_feat,
                 float* item_feat, float* loss, void* stream);

/* Backward of the last train-mode dcue_forward on the same ws: loss.backward() (nn/dcue.py:208).
 * dscores == NULL: gradient of the hinge loss; else dL/dscores [B][N] from the caller.
 * Writes m->grads (dense, overwritten) and the compact embedding gradient (emb_grad/emb_slot),
 * scaled by emb_grad_scale (1/world_size under user-sharded data parallelism). */
int dcue_train_backward(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws,
                        size_t ws_bytes, const float* dscores, float emb_grad_scale, void* stream);

/* ------------------------------------------------------------ DCBR path (BASELINE config 5)
 * The reference never published it (dcrecommend/dcbr is git-ignored, .gitignore:13;
 * nn/dcue_orig.py:35 imports it and fails), so these restate the papers and are parity-unpinned
 * against the reference (pinned against oracle/wrmf_oracle.py and the fp64 oracle item tower).
 *
 * WRMF (Hu, Koren, Volinsky 2008) half-step: every row r of `solve` [n_rows][dim] becomes
 *   x_r = (F^T F + sum_{j in r} (c_rj - 1) f_j f_j^T + lambda I)^{-1} sum_{j in r} c_rj f_j,
 *   c_rj = 1 + alpha * v_rj (v = values, or 1 when values == NULL),
 * with F = `fixed` [n_fixed][dim] and row r's observed columns indices[indptr[r] .. indptr[r+1]).
 * Rows without an observed column get x_r = 0. dim <= 128; lambda > 0. Alternate users and items
 * (the item-side CSR is the transpose) for the ALS iterations. fp64 throughout: rows with at most
 * 32 observed columns through the Woodbury identity over (F^T F + lambda I)^{-1}, the others by a
 * block Cholesky (fp64 MFMA). The workspace holds the Gram partials, G, and that inverse. */
int dcue_wrmf_workspace_bytes(int32_t dim, int64_t n_fixed, size_t* bytes_host);
int dcue_wrmf_half_step(float* solve, int64_t n_rows, const float* fixed, int64_t n_fixed, int32_t dim,
                        const int64_t* indptr, const int32_t* indices, const float* values, float alpha,
                        float lambda, void* ws, size_t ws_bytes, void* stream);
/* DCBR regression step (van den Oord, Dieleman, Schrauwen 2013): the item tower's train forward over
 * the batch's items (catalogue layout, n_neg = 0, n_rows = n_items = M; users unused), the MSE loss
 * mean over [M][d] of (f - target)^2 (torch.nn.MSELoss; target [M][d_s] rows, columns past d
 * ignored) into *loss (device, nullable), and its backward into the item tower's gradients in
 * m->grads (the user-tower segments are left as they are). Workspace: dcue_workspace_bytes(dims, M,
 * 0, M). BN running statistics update as in dcue_forward. */
int dcue_dcbr_step(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, const float* target,
                   float* loss, void* ws, size_t ws_bytes, void* stream);

/* optimizer.step() (nn/dcue.py:209, torch.optim.Adam semantics): dense params + every user row
 * (rows without a gradient this step still decay their moments and move, as the reference's dense
 * embedding gradient does), then clears emb_slot and refreshes wpack. In deferred mode the user
 * table part steps the batch's rows now and records the step for the others (dcue_emb_log); steps
 * must then be consecutive (a->step == step_done + 1). */
int dcue_adam_step(const dcue_model* m, const dcue_adam_args* a, void* stream);

/* The trainer's other optimizers, DCUE(optimize='sgd' | 'ranger') (nn/dcue.py:148-157): one step
 * over the dense flat buffer and every user-table row (the dense embedding gradient: rows outside
 * the batch step with g = 0), then the conv-weight repack. Per-element arithmetic as torch's CPU
 * kernels round it (oracle/optim_oracle.py), sqrt correctly rounded. */
#define DCUE_OPT_SGD 1    /* torch.optim.SGD(lr, momentum=beta1, weight_decay, nesterov=True) */
#define DCUE_OPT_RANGER 2 /* optim/ranger.py:26-165: RAdam + Lookahead */
typedef struct dcue_opt_args {
  int32_t kind;           /* DCUE_OPT_* */
  int32_t step;           /* step count after increment (1 on the first step) */
  double lr, beta1, beta2, eps, weight_decay; /* SGD: beta1 = momentum; beta2, eps unused */
  double alpha;           /* Ranger: lookahead interpolation (0.5 in the trainer) */
  int32_t k;              /* Ranger: lookahead period (6) */
  int32_t reserved;
  double n_sma_threshold; /* Ranger: RAdam rectification threshold (5) */
  double grad_div;        /* as dcue_adam_args.grad_div */
} dcue_opt_args;
/* Optimizer state, caller-owned, zero-initialised before the first step except the lookahead
 * buffers, which start as copies of the parameters (optim/ranger.py:113-114).
 *   SGD: a = momentum buffer.   Ranger: a = exp_avg, b = exp_avg_sq, c = slow (lookahead) weights.
 * dense_*: [n_dense] like params; emb_*: [n_users][E] like the user table. */
typedef struct dcue_opt_state {
  float *dense_a, *dense_b, *dense_c;
  float *emb_a, *emb_b, *emb_c;
} dcue_opt_state;
int dcue_optimizer_step(const dcue_model* m, const dcue_opt_args* a, const dcue_opt_state* st, void* stream);

/* Deferred user-table Adam: log size for a `cap`-step history; (re)initialise the log and row
 * clocks at Adam step `step` (table and moments current to it); bring `users`' rows current;
 * bring every row current (the state then equals the dense sweep's bit for bit). */
int dcue_emb_log_bytes(int32_t cap, size_t* bytes_host);
int dcue_emb_log_init(const dcue_model* m, int32_t cap, int32_t step, void* stream);
int dcue_embedding_sync(const dcue_model* m, const int64_t* users, int32_t n, void* stream);
int dcue_embedding_flush(const dcue_model* m, void* stream);

/* Eval-mode item tower (running BN stats): DCUENet.conv(X) under model.eval() (nn/dcue.py:663).
 * item_feat: [n_items][d_s]. */
int dcue_item_tower_eval(const dcue_model* m, const dcue_tracks* t, const int32_t* item_track,
                         int32_t n_items, void* ws, size_t ws_bytes, float* item_feat, void* stream);
/* Eval user tower: DCUENet.user_embd(idx) (nn/dcue.py:638). user_feat: [n][d_s]. */
int dcue_user_tower(const dcue_model* m, const int64_t* users, int32_t n, void* ws, size_t ws_bytes,
                    float* user_feat, void* stream);

/* Layout conversion of caller-provided spectrograms: [M][128][131] (the reference's per-track tensor,
 * datasets/dcuedataset.py:234-235) -> [M][131][128] track rows (the table layout). */
int dcue_transpose_spectrograms(const float* ncl, int32_t M, float* out, void* stream);
/* Catalogue batch assembly (datasets/dcuedataset.py:242-250 + dcue/dcue.py:90 concat order):
 * item_track = [pos_items[0..B); neg_items[b][j] at B + b*N + j]. */
int dcue_build_catalogue_batch(const int64_t* pos_items, const int64_t* neg_items, int32_t B,
                               int32_t N, int32_t* item_track, void* stream);

/* ------------------------------------------------------------------------------ samplers */
/* MT19937 state (numpy legacy RandomState): 624 words + position, in device memory. */
typedef struct dcue_mt_state {
  uint32_t key[624];
  int32_t pos;
  int32_t pad[3];
} dcue_mt_state;

/* np.random.seed(seed) into a device state (init_genrand). */
int dcue_mt_seed(dcue_mt_state* state, uint32_t seed, void* stream);
/* n tempered 32-bit outputs, advancing the state (genrand_int32). */
int dcue_mt_draw(dcue_mt_state* state, uint32_t* out, int32_t n, void* stream);
/* In-batch negatives (nn/dcue.py:698-709): neg[b][j] = masked draw over the B-1 other rows, from
 * one global stream, row-major. Bit-exact with numpy for the same state. */
int dcue_sample_inbatch(dcue_mt_state* state, int32_t B, int32_t N, int32_t* neg, void* stream);
/* Catalogue negatives (datasets/dcuedataset.py:207-220): for each sample the user's non-items in
 * the split (split_items sorted; user_split_rank = CSR over users of the ranks, inside split_items,
 * of the user's split items, sorted), N draws with replacement. reseed != 0: every sample draws from
 * a fresh stream seeded with `seed` (random_seed mode); else all samples share `state` in order.
 * Writes item ids (values of split_items). A user with no non-item in the split (numpy raises
 * ValueError there) gets a row of -1 and consumes no draw: callers check for such users on the host
 * (their CSR row length >= n_split) and raise before sampling them; dcue_build_catalogue_batch
 * maps a -1 to item 0 so it never reads outside the track table. */
int dcue_sample_catalogue(dcue_mt_state* state, int32_t reseed, uint32_t seed,
                          const int64_t* split_items, int64_t n_split, const int64_t* user_indptr,
                          const int32_t* user_split_rank, const int64_t* users, int32_t n_samples,
                          int32_t N, int64_t* out, void* stream);

/* (added under ABI 17) Catalogue negatives drawn in proportion to integer weights. w[p] (uint32,
 * zeros allowed) is the weight of split position p, W = sum(w) <= 2^32 - 1. For one sample of user u,
 * with cand the split positions that are not the user's, ascending:
 *   cw = cumsum(w[cand]);  W_u = cw[-1];  r = np.random.randint(0, W_u, N)   (legacy RandomState)
 *   out = split_items[cand[searchsorted(cw, r, side='right')]]
 * bit for bit: every draw is one bounded integer of the masked-rejection stream dcue_sample_catalogue
 * consumes, and the map from a draw to an item is integer arithmetic. A zero-weight song is never
 * drawn. W_u == 0 (numpy raises ValueError): the row is -1 and consumes no draw; callers check on the
 * host first. W_u == 1 consumes no draw either. w == 1 everywhere reproduces dcue_sample_catalogue:
 * the same outputs and the same state afterwards.
 * The tables are device arrays built once per dataset from (user_indptr, user_split_rank, w), with
 * rank_e the user's e-th split rank (datasets/csr.py weighted_split_tables builds them):
 *   cum[n_split + 1]     cum[p] = w[0] + ... + w[p-1]                       (cum[n_split] = W)
 *   user_skip[nnz]       by CSR entry: E_e = w[rank_0] + ... + w[rank_{e-1}] within the user's list
 *   user_key[nnz]        by CSR entry: K_e = cum[rank_e] - E_e, non-decreasing within a list
 *   user_weight[n_users] W_u = W - (the sum of w over the user's list)
 * Both protocols of dcue_sample_catalogue and its other arguments; N <= 1024. */
typedef struct dcue_weight_tables {
  const uint32_t* cum;
  const uint32_t* user_key;
  const uint32_t* user_skip;
  const uint32_t* user_weight;
} dcue_weight_tables;
int dcue_sample_catalogue_weighted(dcue_mt_state* state, int32_t reseed, uint32_t seed,
                                   const int64_t* split_items, int64_t n_split,
                                   const int64_t* user_indptr, const int32_t* user_split_rank,
                                   const dcue_weight_tables* tables, const int64_t* users,
                                   int32_t n_samples, int32_t N, int64_t* out, void* stream);

/* (added under ABI 17) Hard negatives: out of a pool of P sampled candidates per row, keep the H that
 * the given factors score highest for the row's user, and fill the row up to N with the pool's other
 * draws in the order they were drawn (dynamic negative sampling).
 *   user_feat [n_users][d], item_feat [n_items][d]: fp32, dense rows of exactly d floats, 1 <= d <= 256
 *     (d need not be a multiple of 4: rows of d = 30 are only 8-byte aligned);
 *   users [n_samples]; pool [n_samples][P]: item indices as dcue_sample_catalogue* writes them;
 *   out [n_samples][N], out_hard [n_samples], out_flags [n_samples].
 * Score of pool position p for row b: nn.CosineSimilarity's u.c / (max(|u|, 1e-8) * max(|c|, 1e-8)) in
 * fp32, a function of the two rows' values only -- not of p, b, P, N, H, n_samples or how rows are
 * batched. Splitting a call's rows over several calls therefore gives the same bits, and item rows
 * that are bitwise equal tie exactly (-0 and +0 are one score).
 * Hard set: a position is eligible when its id is in [0, n_items), it is the first occurrence of that
 * id in the row, and its score is not NaN. The h = min(H, #eligible) best eligible positions by (score
 * descending, position ascending) are hard; out[b][0:h] holds their ids in ascending pool position and
 * out_hard[b] = h.
 * Fill: out[b][h:N] holds the first N - h pool positions not chosen as hard, in pool order, ids copied
 * as they are: duplicates and -1 pass through (dcue_build_catalogue_batch maps -1 to item 0). H = 0
 * returns pool[b][0:N], and the fill is distributed as the base sampler's draws.
 * out_flags[b]: DCUE_SELECT_FLAG_NONFINITE a score was NaN or infinite; DCUE_SELECT_FLAG_BAD_ID an id
 * was outside [0, n_items) -- such an id is never hard and never addresses item_feat -- or the row's
 * user id was outside [0, n_users), and the row then has h = 0.
 * Required: 1 <= N <= P <= DCUE_SELECT_MAX_POOL, 0 <= H <= N, n_samples >= 0 (0 is a no-op success).
 * Every argument is validated on the host before the first device call (DCUE_ERR_INVALID: a null
 * pointer, a negative count, d < 1, N, P or H out of range; DCUE_ERR_UNSUPPORTED: d > 256). No
 * workspace. The call does not synchronise `stream`: the trainer runs it on its sampling stream, two
 * steps ahead of the step that consumes the row. */
#define DCUE_SELECT_MAX_POOL 1024
#define DCUE_SELECT_FLAG_NONFINITE 1
#define DCUE_SELECT_FLAG_BAD_ID 2
int dcue_select_negatives(const float* user_feat, int64_t n_users, const float* item_feat, int64_t n_items,
                          int32_t d, const int64_t* users, const int64_t* pool, int32_t n_samples,
                          int32_t P, int32_t N, int32_t H, int64_t* out, int32_t* out_hard,
                          int32_t* out_flags, void* stream);

/* -------------------------------------------------------------------------- step plans */
/* A training-step plan: the step's kernels (optionally the in-batch negative draw, then the train
 * forward and backward of dcue_forward/dcue_train_backward) bound once and issued by one host call
 * per step. The model, batch, tracks and workspace buffers are bound at creation (their addresses
 * must stay valid and unchanged); their CONTENTS are read at each launch, so the caller refreshes
 * the batch buffers between launches (or passes sources to dcue_plan_launch, which copies them in
 * stream order first). The optimizer step stays outside (its scalars change every step), as does
 * any gradient all-reduce between the two. Replay is eager (issued from C++ onto the caller's
 * stream + side streams) unless DCUE_PLAN_GRAPH asks for a captured HIP graph. */
typedef struct dcue_plan dcue_plan;
#define DCUE_PLAN_SAMPLE_INBATCH 1 /* step starts with dcue_sample_inbatch(mt, B, N, b->neg_item) */
#define DCUE_PLAN_GRAPH 2          /* capture into a HIP graph and replay that */
typedef struct dcue_plan_config {
  int32_t flags;        /* DCUE_PLAN_* */
  float margin;         /* hinge margin (nn/dcue.py:167-170) */
  float emb_grad_scale; /* as dcue_train_backward */
  int32_t reserved;
  dcue_mt_state* mt;    /* sampler state (DCUE_PLAN_SAMPLE_INBATCH) */
} dcue_plan_config;
int dcue_plan_create(const dcue_model* m, const dcue_batch* b, const dcue_tracks* t, void* ws,
                     size_t ws_bytes, const dcue_plan_config* cfg, dcue_plan** plan_host);
/* users_src / item_track_src (nullable): copied into the bound batch buffers before the replay. */
int dcue_plan_launch(dcue_plan* plan, const int64_t* users_src, const int32_t* item_track_src,
                     void* stream);
/* dcue_plan_launch, then (adam != NULL) dcue_adam_step on the plan's model: one host call per
 * training step (a bound communicator's exchange included, dcue_plan_set_comm). Without a
 * communicator the dense Adam is split: bn0 / conv 1 / bn1 on `stream` right behind the conv-1
 * weight gradient, the other segments on the library's user stream once the side streams'
 * gradients are in, so `stream` never waits for that join; the plan's next launch waits for it
 * before conv 2. Until then the parameters are current only for work ordered after dcue_plan_sync
 * (every library entry point that reads them joins by itself). */
int dcue_plan_step(dcue_plan* plan, const int64_t* users_src, const int32_t* item_track_src,
                   const dcue_adam_args* adam, void* stream);
/* `stream` waits for everything the plan's last step left on the library's side streams. */
int dcue_plan_sync(dcue_plan* plan, void* stream);
/* Data-parallel overlap (row e): `stream` waits until every side-stream part of the plan's last
 * launched step is in. From then on the flat gradient buffer is final except its first
 * DCUE_SEG_LATE segments (bn0, conv layer 1, bn1: written by the caller's stream at the step's end),
 * so an all-reduce of the rest issued on `stream` overlaps the conv-1 weight gradient. Eager plans
 * only (DCUE_ERR_INVALID for a graph plan or before the first launch). Replaces the single
 * post-backward all-reduce of the DDP-style loop (nn/dcue.py:208-209 under data parallelism). */
#define DCUE_SEG_LATE 6
int dcue_plan_wait_side(dcue_plan* plan, void* stream);
/* Lookahead (eager plans of a BatchNorm tower): announces the item_track_src buffer of the
 * NEXT launch ([M] int32 device ids, contents fixed until that launch). The following launch then
 * also prepares that batch's model-independent item inputs beside its own step -- bn0's batch
 * statistics (k_input_stats) and bn0(x) zero-padded for the conv-1 weight gradient (k_xhat0) -- so
 * the next step's chain starts at conv 1. A next launch whose item_track_src is not the announced
 * buffer computes them itself, as without lookahead; NULL withdraws the announcement. The batch
 * composition of the reference is likewise prepared ahead, by its DataLoader workers
 * (nn/dcue.py:711-721). The announced items must be written, in `stream` order, before the
 * announcing launch (the lookahead reads them after that launch's score kernel, on a side stream).
 * DCUE_ERR_UNSUPPORTED for graph or BatchNorm-free plans. */
int dcue_plan_set_next(dcue_plan* plan, const int32_t* next_item_track);

/* ---- check mode (a HIP bounds/NaN check mode; the reference has none) ----
 * Probes run between steps. Each ORs `bit` into the device word *flags when it finds a problem and
 * never faults on the data it inspects: ids can be validated before a step indexes with them, and
 * the loss, parameters, gradients and user table after it. */
int dcue_check_finite(const float* buf, int64_t n, int32_t* flags, int32_t bit, void* stream);
/* ids: int32 (id_bytes 4) or int64 (8); flags any id outside [0, limit). */
int dcue_check_ids(const void* ids, int32_t id_bytes, int64_t n, int64_t limit, int32_t* flags, int32_t bit,
                   void* stream);
int dcue_plan_destroy(dcue_plan* plan);

/* ---- debug: schedule perturbation, probes, poison (no reference counterpart) ----
 * dcue_debug_delay: every later step launches, ahead of the work at `site`, a spin kernel of
 * `microseconds` (0: none, at most 1e6) on that work's stream. A step's results are bit-identical
 * under any delays -- every buffer is ordered by the streams' events, not by timing -- so a
 * difference names a missing cross-stream wait (tests/test_gpu_races.py). */
#define DCUE_SITE_USER_FWD 0   /* user stream: the user tower's forward (deferred-row sync + GEMMs) */
#define DCUE_SITE_USER_BWD 1   /* user stream: the user tower's backward + user-table Adam */
#define DCUE_SITE_WGRAD_HI 2   /* wgrad stream 0: weight gradients of conv layers 3-5 (+ fc) */
#define DCUE_SITE_WGRAD_2 3    /* wgrad stream 1: weight gradient of conv layer 2 */
#define DCUE_SITE_FC_WGRAD 4   /* wgrad stream 1: res / text towers' fc (+ text conv) weight gradients */
#define DCUE_SITE_LATE_ADAM 5  /* split plans: the late segments' Adam (user or comm stream) */
#define DCUE_SITE_PROLOGUE 6   /* plans: the next step's prologue (wgrad stream 0) */
#define DCUE_SITE_LOOKAHEAD 7  /* plans: the announced next batch's input statistics (wgrad stream 0) */
#define DCUE_SITE_CONV2 8      /* caller's stream: conv 2 forward */
#define DCUE_SITE_DGRAD_2 9    /* caller's stream: conv-2 input gradient (g1) */
#define DCUE_SITE_WGRAD_1 10   /* caller's stream: conv-1 weight gradient */
#define DCUE_SITE_TEXT_FWD 11  /* text tower: the text branch's forward on its side stream (ABI 16) */
/* (added under ABI 17: appended, nothing earlier changes) the backward's two fork points */
#define DCUE_SITE_DGRAD_4 12   /* caller's stream: conv-4 input gradient (g3) */
#define DCUE_SITE_DGRAD_3 13   /* caller's stream: conv-3 input gradient (g2) */
#define DCUE_N_DEBUG_SITES 14
int dcue_debug_delay(int32_t site, int32_t microseconds);
/* Probes: buf = NULL (off) or a device array of dcue_debug_probe_count() records
 * { uint32 nonfinite; uint32 nonzero; uint64 first_bad } (the caller sets first_bad to UINT64_MAX
 * and the rest to 0). While bound, steps check the output of each probed launch on its own stream
 * (no added cross-stream order): a non-finite element sets `nonfinite` and takes the minimum of the
 * device's 100 MHz wall clock into `first_bad`; any non-zero element sets `nonzero`. The record with
 * the smallest first_bad names the first launch that wrote a non-finite value. */
int dcue_debug_probes(void* buf);
int dcue_debug_probe_count(void);
const char* dcue_debug_probe_name(int32_t i);
/* on != 0: plans created afterwards fill the scratch they allocate with 0xFF bytes (float NaN). */
int dcue_debug_poison(int32_t on);
/* Reads and clears the current device's word that the fused user-tower forward sets when a bounded
 * wait for another workgroup's row gave up (bit 0; never expected). bench.py fails its line on a
 * non-zero value. */
int dcue_debug_fail_flags(uint32_t* flags_host);
/* ORs `bits` into the current device's fail word (tests: a forced flag must fail the bench line; ABI 16). */
int dcue_debug_raise_fail_flags(uint32_t bits);
/* Which kernel variants a training step of this shape launches (added under ABI 17; host only: no
 * device call, works without a GPU). The launchers pick tilings, split-K partitions and kernels from
 * the item count M (and the score kernel from N); this reports those picks from the very functions
 * the launches call, so a test can tell which variants its shapes reach (tests/test_launch_shapes_cpu.py).
 * layout, B, N, M as in dcue_batch (catalogue: M = B(1+N); gather: M >= B, copy lists as the step's);
 * the track table is taken as fp16. out_host gets DCUE_LAUNCH_SHAPE_WORDS int32 words (cap: its size):
 *   [0, 25)   conv forward 1..5, 5 words each: TW (row tiles per workgroup), DEEP, split-f16,
 *             rows of the last workgroup (M R mod 16 TW; 0: full), a workgroup spans two items
 *   [25, 45)  input gradient of layers 2..5, the same 5 words
 *   [45, 69)  weight gradient of layers 1..6 (6: the fc), 4 words each: kernel (0 k_conv_wgrad16t
 *             tap-fused split-f16, 1 k_conv_wgrad16 kc-tiled split-f16, 2 k_conv_wgrad f32, 3
 *             k_conv1_wgrad, 4 / 5 the multi-layer launch split-f16 / f32, 6 k_conv_wgrad1k; -1: none,
 *             the res / text towers' fc), nchunk, rows_per_chunk, rows of the last chunk
 *   [69, 74)  k_score_fused's CPW (0: the general one), item-gradient kernel (0 k_item_grad_multi, 1
 *             k_item_grad), its items per workgroup IT, WLDS, items of its last workgroup */
#define DCUE_LAUNCH_SHAPE_WORDS 74
int dcue_debug_launch_shape(const dcue_dims* dims, int32_t layout, int32_t B, int32_t N, int32_t M,
                            int32_t* out_host, int32_t cap);
/* The text branch's launches over M items (text tower only; added under ABI 17; host only), from the
 * functions launch_text_fwd / launch_text_wgrad call, with the A/B knobs unset. out_host gets
 * DCUE_TEXT_SHAPE_WORDS int32 words (cap: its size):
 *   [0]  forward kernel: 0 k_text_fwd_full (an item's sentence staged once), 1 k_text_fwd (chunked:
 *        where the staged sentence would not fit 150 KB of LDS)
 *   [1]  16-position tiles per workgroup (TBW / TB)     [2]  full: waves; chunked: items per workgroup
 *   [3]  column tiles per wave (NCT)                    [4]  full: B steps in flight (BPD); chunked: 0
 *   [5]  compile-time K chunks (NCH; 0: run time)       [6]  full: XCDs the units run on; chunked: 0
 *   [7]  full: (item, column block) units; chunked: workgroups
 *   [8]  blocks launched                                [9]  dynamic LDS bytes
 *   [10] static LDS bytes                               [11] items of the last workgroup along M
 *   [12] weight-gradient chunks                         [13] items per chunk
 *   [14] items of the last chunk                        [15] 1: k_text_wreduce runs */
#define DCUE_TEXT_SHAPE_WORDS 16
int dcue_debug_text_shape(const dcue_dims* dims, int32_t M, int32_t* out_host, int32_t cap);

/* ------------------------------------------------- data-parallel gradient exchange (RCCL) */
/* One process per GPU; users are sharded over the ranks, so the only exchange of a step is the
 * mean over ranks of the replicated dense gradient (the flat buffer, dcue_param_layout). The
 * library drives RCCL itself so that a data-parallel step stays one host call (dcue_plan_step).
 * The caller ships the unique id from rank 0 to the others (e.g. over torch.distributed). */
typedef struct dcue_comm dcue_comm;
#define DCUE_COMM_ID_BYTES 128
int dcue_comm_unique_id(void* id_host); /* rank 0: DCUE_COMM_ID_BYTES bytes */
/* A communicator over `world` ranks on the current HIP device (collective: every rank calls it). */
int dcue_comm_create(const void* id_host, int32_t world, int32_t rank, dcue_comm** comm_host);
/* A communicator whose transport is the caller's: `fn(ctx, host_buf, n, dtype)` must replace the n
 * elements at host_buf (DCUE_COMM_F32: float, DCUE_COMM_U64: uint64, two's-complement wrap) by their
 * sum over the ranks and return 0. The library drains its stream and stages the buffer through pinned
 * host memory around each call, so a plan step blocks the host at every exchange point; it runs the
 * same exchange code (buckets, event order, Adam's divide) as the RCCL transport. For ranks that
 * cannot share an RCCL communicator -- several ranks on one GPU over gloo (tests) -- not for speed. */
#define DCUE_COMM_F32 0
#define DCUE_COMM_U64 1
typedef int (*dcue_host_allreduce_fn)(void* ctx, void* host_buf, int64_t n, int32_t dtype);
int dcue_comm_create_host(int32_t world, int32_t rank, dcue_host_allreduce_fn fn, void* ctx,
                          dcue_comm** comm_host);
int dcue_comm_destroy(dcue_comm* comm);
/* In-place mean over the ranks of n floats, ordered on `stream` (sum all-reduce, then / world). */
int dcue_comm_allreduce_mean(dcue_comm* comm, float* buf, int64_t n, void* stream);
/* In-place all-gather, ordered on `stream`: buf holds world * count floats, rank r's own part at
 * buf[r * count, (r + 1) * count); afterwards every rank holds every part (RCCL: ncclAllGather; the
 * host transport: the other parts zeroed, then the sum). The DCBR path's row-sharded WRMF half-steps
 * (each rank solves its rows, every rank needs all of them as the next half-step's fixed side). */
int dcue_comm_allgather(dcue_comm* comm, float* buf, int64_t count, void* stream);
/* Bind (or, with NULL, unbind) a communicator to an eager plan. dcue_plan_step then exchanges the
 * dense gradient between the backward and Adam, in two buckets on the communicator's stream: the
 * gradients the side streams finish (everything after DCUE_SEG_LATE) as soon as they are in,
 * overlapping the conv-1 weight gradient on the caller's stream, then bn0/conv-1/bn1 once the step
 * ends; Adam then divides by the world size (dcue_adam_args.grad_div) in its sweep. dcue_plan_launch
 * makes the same exchange and divides by the world size itself, so the gradient it leaves is the
 * mean over the ranks for any optimizer called after it (dcue_optimizer_step, dcue_adam_step with
 * grad_div 0). Collective order is the same on every rank. The plan must have been created with
 * emb_grad_scale = 1/world. */
int dcue_plan_set_comm(dcue_plan* plan, dcue_comm* comm);
/* SyncBN (on != 0; the bound communicator's ranks): every train-mode BatchNorm of the item
 * tower normalises over the whole global batch. Its exact fixed-point sums (forward: count-weighted
 * sum and sum of squares; backward: sum g and sum g*xhat) are all-reduced over the ranks between
 * their producer and first consumer, so the statistics -- and the running statistics -- are the same
 * on every rank and do not depend on the order of the ranks. BN gamma/beta gradients enter the
 * exchange as 1/world of the global sum each, so after the DDP mean they equal torch
 * SyncBatchNorm + DDP's (the mean of the per-rank local sums). 11 small collectives per step (6 BN
 * layers forward, bn5..bn1 backward; bn0 has no input gradient, its gamma/beta gradients stay local).
 * Requires a bound communicator (DCUE_ERR_INVALID otherwise) and the split-f16 weight gradients
 * (DCUE_ERR_UNSUPPORTED under DCUE_WGRAD_F16=0). Unbinding the communicator turns it off. */
int dcue_plan_set_sync_bn(dcue_plan* plan, int32_t on);

/* ------------------------------------------------------------------- live kernel timing */
/* enable = n > 0: every n-th launch of the kernel class (also inside plans created afterwards),
 * starting with the n-th after this call (ABI 16), gets a HIP event pair bound to the launch itself
 * (its dispatch's start and end); 0 disables.
 * dcue_timer_read waits for the recorded pairs, returns their summed time and count, and resets.
 * For bench rooflines: a timed launch costs the stream a few microseconds, so time a sample. */
#define DCUE_TIMED_CONV1_WGRAD 0 /* conv layer-1 weight gradient (the step's largest MFMA kernel) */
#define DCUE_TIMED_CONV1_FWD 1   /* conv layer-1 forward */
#define DCUE_TIMED_EMB_FLUSH 2   /* deferred user-table Adam: full-table flush */
#define DCUE_TIMED_ADAM_EMBED 3  /* dense user-table Adam sweep */
#define DCUE_TIMED_ALLREDUCE 4    /* a plan's RCCL gradient exchange (each bucket's all-reduce) */
#define DCUE_TIMED_EMB_SLICE 5    /* deferred user-table Adam: one step's rolling-flush slice */
#define DCUE_TIMED_TEXT_FWD 6     /* text tower: the text conv forward (k_text_fwd, config 4) */
#define DCUE_TIMED_USER_FWD 7     /* the fused user-tower forward (k_user_fwd; ABI 16) */
#define DCUE_TIMED_TEXT_WGRAD 8   /* text tower: the text conv's weight gradient (k_text_wgrad; ABI 16) */
#define DCUE_N_TIMED 9
int dcue_timer_enable(int32_t kernel, int32_t enable);
int dcue_timer_read(int32_t kernel, double* total_ms_host, int64_t* launches_host);
/* The same recorded launches one by one: each duration in ms into ms_host[0 .. min(n, cap)), the
 * count into *launches_host; resets (ABI 15). */
int dcue_timer_samples(int32_t kernel, float* ms_host, int64_t cap, int64_t* launches_host);

/* ------------------------------------------------------------------------ evaluation metrics */
/* Ranking metrics of DCUE's evaluation for a batch of queries (users for DCUE.score, songs for
 * DCUE.score_song), replacing the per-query predict() loops and sklearn calls of nn/dcue.py:380-476
 * and the candidate lists of datasets/dcuepredset.py:39-131.
 *   query_feat [n_query_rows][d], cand_feat [n_cand][d]: factors (DCUE.user_factors / item_factors,
 *     nn/dcue.py:629-668); scores are nn.CosineSimilarity(dim=1) of a query row and a candidate row.
 *   queries[n_queries]: query row of each evaluated query (a sample; repeats allowed, :413/:420).
 *   pos_ptr[n_query_rows+1], pos_idx: CSR over query rows of the candidates the query interacted
 *     with in ANY split (datasets/dcuedataset.py:74-89 item_user matrix), each row sorted, no repeats.
 *   cand_class[n_cand]: bit 0 = the candidate is in the pred list (the pred split's songs/users),
 *     bit 1 = in the truth list; 0 = in neither.
 *   DCUE_RANK_SPLIT (DCUE.score, :399-447): AUC weighted over {pred positives + truth negatives} and
 *     {pred negatives + truth positives}, AP over both; has_pos = the query has pred positives (the
 *     reference stops its user loop at the first query without, :393-394).
 *   DCUE_RANK_SINGLE (DCUE.score_song, :463-474): targets = 1 for the query's positives among the
 *     candidates with bit 1, 0 for EVERY candidate with bit 0 -- positives included: the reference's
 *     non-user list (dcuepredset.py:53-62) takes `getrow(i).nonzero()[0]`, the row indices (all 0),
 *     so it only drops user index 0 and keeps the song's own users as negatives too; callers set
 *     bit 0 on the split's users except user 0 and bit 1 on the split's users. AUC / AP over that
 *     list, 1/1 if every target is 1, 0/0 if none; has_pos = 0 marks a query the reference skips.
 *   has_pos bit 1: a score the reference would hand to sklearn is NaN or infinite -- there
 *     roc_auc_score / average_precision_score raise ValueError (:440, :447, :473-474), and the
 *     query's auc / ap here are meaningless (the binding raises ValueError instead of using them).
 * Exact tie-aware AUC (Mann-Whitney, ties 1/2) and step-wise AP from integer rank counts, fp64.
 * At most 4096 positives per query inside the lists (else DCUE_ERR_UNSUPPORTED). query_batch
 * queries are scored per pass; the workspace holds their [query_batch][n_cand] score rows.
 * auc, ap and has_pos do not depend on query_batch, bit for bit: a score is one dot product in a
 * summation order that depends on d alone, the counts are integers, and the fp64 sums of a query
 * run in one fixed order.
 * Synchronises `stream` before returning. */
#define DCUE_RANK_SPLIT 0
#define DCUE_RANK_SINGLE 1
int dcue_rank_workspace_bytes(int64_t n_cand, int32_t d, int32_t query_batch, size_t* bytes_host);
int dcue_rank_metrics(const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                      int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries,
                      const int64_t* pos_ptr, const int32_t* pos_idx, const uint8_t* cand_class,
                      int32_t mode, int32_t query_batch, void* ws, size_t ws_bytes, double* auc,
                      double* ap, int32_t* has_pos, void* stream);
/* DCUE._item_factors' averaging (nn/dcue.py:655-668): f <- (f + f + ... n_iter times) / n_iter in
 * fp32. It stands for the n_iter eval passes only where they are identical: a catalogue without a
 * full-length store (the table was cropped once, at load), or one whose tracks all have at most 131
 * frames. With a store bound the trainer runs n_iter real passes over dcue_crop_tracks windows and
 * accumulates them itself (DCUE._factors_over). */
int dcue_factor_repeat_mean(float* f, int64_t n, int32_t n_iter, void* stream);

/* ------------------------------------------------------------------- top-K recommendation (ABI 17) */
/* The k best candidates of each query by nn.CosineSimilarity(dim=1), without the score matrix:
 * what a recommender serves ("the K tracks for this user"; item-to-item with the item factors on
 * both sides). Scores are dcue_rank_metrics' -- the same normalisation (x / max(||x||, 1e-8)) and the
 * same exact-f32 MFMA summation order, which depends on d alone -- so the lists do not depend on
 * query_batch or cand_split, bit for bit.
 *   query_feat [n_query_rows][d], cand_feat [n_cand][d], queries[n_queries]: as dcue_rank_metrics
 *     (repeats allowed). d <= 256, else DCUE_ERR_UNSUPPORTED.
 *   excl_ptr[n_query_rows+1], excl_idx: CSR over query rows of candidates never to return for the
 *     query (what the user already played), each row sorted, no repeats; both null: no exclusion.
 *   cand_mask[n_cand]: 0 = never return the candidate; null: every candidate.
 *   Candidate c is eligible for a query when its mask byte is non-zero, it is not in the query's
 *     exclusion row and its score is not NaN. Order: score descending, then index ascending.
 *   out_idx / out_score [n_queries][k], best first; where fewer than k candidates are eligible the
 *     tail is idx -1 / score -inf, and out_count[q] says how many entries are real.
 *   out_flags[q] bit 1: an eligible candidate's score is NaN or infinite (non-finite factors: a
 *     diverged model). A NaN is never returned; +-inf order as ordinary values.
 *   1 <= k <= DCUE_TOPK_MAX_K. query_batch queries are ranked per pass. cand_split: candidate chunks a
 *     query tile is divided over, each leaving k partial keys that a merge kernel combines -- 0: the
 *     library chooses (enough workgroups to fill the chip); positive: forced (at most 32, and at most
 *     one per 64 candidates).
 *   Workspace: both sides' normalised rows and the partial keys, (queries of a pass) x cand_split x
 *     k x 8 bytes -- never a [query_batch][n_cand] buffer. dcue_topk_workspace_bytes is a host
 *     computation, and dcue_topk validates every argument on the host before its first device call.
 * Synchronises `stream` before returning. */
#define DCUE_TOPK_MAX_K 128
int dcue_topk_workspace_bytes(int64_t n_cand, int32_t d, int32_t query_batch, int32_t k,
                              int32_t cand_split, size_t* bytes_host);
int dcue_topk(const float* query_feat, int64_t n_query_rows, const float* cand_feat, int64_t n_cand,
              int32_t d, const int32_t* queries, int32_t n_queries, const int64_t* excl_ptr,
              const int32_t* excl_idx, const uint8_t* cand_mask, int32_t k, int32_t query_batch,
              int32_t cand_split, void* ws, size_t ws_bytes, int32_t* out_idx, float* out_score,
              int32_t* out_count, int32_t* out_flags, void* stream);
/* (added under ABI 17) dcue_topk with the score chosen by the caller -- every other argument, the
 * workspace (dcue_topk_workspace_bytes) and every rule above unchanged:
 *   DCUE_SCORE_COSINE: dcue_topk itself (dcue_topk is this call with that value; same bits).
 *   DCUE_SCORE_DOT: the plain inner product of the raw rows, q . c -- what a matrix factorisation
 *     (WRMF: x_u . y_i) ranks by, where the row norms carry the popularity the cosine divides out.
 *     The two prep passes gather and zero-pad the rows without scaling them; the score kernel, the
 *     keys, the selection, eligibility, the tie order, the padding of short lists and out_count are
 *     dcue_topk's, and so is the summation order (it depends on d alone): the lists do not depend on
 *     query_batch or cand_split, bit for bit. out_flags bit 1 keeps its meaning; a dot product of
 *     large finite factors can overflow where a cosine cannot, and then sets it too. +-inf order as
 *     ordinary values, a NaN is never returned.
 * Any other `score` is DCUE_ERR_INVALID, on the host before the first device call. */
#define DCUE_SCORE_COSINE 0
#define DCUE_SCORE_DOT 1
int dcue_topk_scored(int32_t score, const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                     int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries,
                     const int64_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand_mask, int32_t k,
                     int32_t query_batch, int32_t cand_split, void* ws, size_t ws_bytes, int32_t* out_idx,
                     float* out_score, int32_t* out_count, int32_t* out_flags, void* stream);
/* (added under ABI 17) dcue_topk_scored with an additive per-candidate prior -- popularity promotion or
 * demotion, editorial boosts, recency, a matrix factorisation's item biases. cand_prior follows
 * cand_mask, the other per-candidate array; every other argument, the workspace
 * (dcue_topk_workspace_bytes: the prior needs none) and every rule above unchanged:
 *   cand_prior float [n_cand] (device), or null: the call is then dcue_topk_scored -- the same kernels,
 *     the same bits.
 *   Score: s = fl32(s0 + cand_prior[c]), where s0 is the score dcue_topk_scored produces for the pair
 *     (its -0 already +0); the sum's -0 is folded to +0 again before keying. It is ONE fp32 addition
 *     after the MFMA accumulators are final, never a term of their sum: s is a function of (s0's bits,
 *     the prior) alone, so the lists still do not depend on query_batch or cand_split, bit for bit.
 *   out_score is the sum, the number the list was ranked by. Key, order (score descending, then index
 *     ascending), mask, exclusion CSR, padding, out_count and the merge are dcue_topk's.
 *   out_flags[q] bit 1: an eligible candidate's SUM is NaN or infinite -- a non-finite s0, a non-finite
 *     prior, or an overflow of the addition. A NaN is never returned; +-inf order as ordinary values. The
 *     prior of a candidate the mask or the query's exclusion row removes is never looked at.
 * Validated on the host before the first device call as dcue_topk_scored is, each refusal with a
 * dcue_last_error text. Synchronises `stream` before returning. */
int dcue_topk_prior(int32_t score, const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                    int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries,
                    const int64_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand_mask,
                    const float* cand_prior, int32_t k, int32_t query_batch, int32_t cand_split, void* ws,
                    size_t ws_bytes, int32_t* out_idx, float* out_score, int32_t* out_count, int32_t* out_flags,
                    void* stream);

/* ------------------------------------------------------------ WRMF objective (added under ABI 17) */
/* The objective the ALS half-steps (dcue_wrmf_half_step) descend,
 *   L = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2),
 * over ALL n_users x n_items pairs (p = 1, c = 1 + alpha v on the observed ones; p = 0, c = 1
 * elsewhere) without the dense matrix: with s_ui = x_u . y_i,
 *   L = sum_{(u,i) observed} [c_ui (1 - s_ui)^2 - s_ui^2]  +  sum_{a,b} (X^T X)_ab (Y^T Y)_ab
 *       +  lambda (tr X^T X + tr Y^T Y)
 * (the middle term is sum_{u,i} s_ui^2 over every pair). Everything in fp64, accumulated from the
 * fp32 factors: the first two terms cancel to a few percent of their size near a fit.
 *   X [n_users][dim], Y [n_items][dim] fp32, dim <= 128; indptr[n_users+1] / indices / values: the
 *     by-user CSR in dcue_wrmf_half_step's format (values null: v = 1). A pair listed twice counts
 *     twice. An index outside [0, n_items) is not dereferenced; it makes the observed term NaN.
 *   out (device) [4] doubles: L, the observed term, the all-pairs term, the regulariser.
 * Every reduction has a fixed order -- a pair's dot product a fixed cross-lane tree, a row's pairs in
 * pair order, the rows a tree whose shape depends on n_users alone, the Grams dcue_wrmf_half_step's
 * -- so two calls give the same bits. Validated on the host before the first device call
 * (DCUE_ERR_INVALID: a null X / Y / indptr / out / ws, indices null with n_users > 0, n_users < 0,
 * n_items < 0, dim outside 1..128, lambda <= 0; DCUE_ERR_WORKSPACE). n_users == 0, n_items == 0 or a
 * CSR without pairs is DCUE_OK: the observed term is 0 and the other two are what the factors give.
 * alpha and lambda are doubles here (dcue_wrmf_half_step rounds its own to fp32: a relative 6e-8 of
 * lambda, which moves its minimiser, and so L, only in second order). Asynchronous on `stream`. Workspace: the Gram partials, both Grams and one double per user. */
int dcue_wrmf_objective_workspace_bytes(int64_t n_users, int64_t n_items, int32_t dim, size_t* bytes_host);
int dcue_wrmf_objective(const float* X, int64_t n_users, const float* Y, int64_t n_items, int32_t dim,
                        const int64_t* indptr, const int32_t* indices, const float* values, double alpha,
                        double lambda, void* ws, size_t ws_bytes, double* out, void* stream);

/* ------------------------------------------------------ fold-in of unseen users (added under ABI 17) */
/* A user outside the trained table -- a new listener, a playlist, a session -- gets a factor without
 * retraining: with the model frozen, one fresh embedding row per new user is learned against the
 * trained towers with the training loss itself (cosine hinge, n_neg sampled negatives per positive)
 * and torch.optim.Adam steps on that row alone. All `steps` steps of every user run in ONE kernel
 * launch (a workgroup keeps 16 users from the first step to the last); the reference has no
 * counterpart (its predict() looks the user up in user_index).
 *   m: read only, and only the user tower's segments of m->params (user_embd.linear1 / linear2).
 *     Nothing in *m is written: not params, not emb, not the moments, not the deferred log.
 *   cand_feat [n_cand][d] (d = dims.feature_dim), cand_mask[n_cand] (nullable: every candidate is
 *     eligible as a negative): dcue_topk's operands.
 *   hist_ptr / hist_idx: dcue_topk's exclusion CSR format (int64 pointers, int32 candidate indices,
 *     ascending and distinct per row), indexed by GLOBAL row r = row0 + local row, so a caller that
 *     chunks its users passes the same arrays to every chunk and to dcue_topk. emb, out_feat,
 *     out_loss, out_grad and out_flags are indexed by the local row 0 .. n_users-1.
 * Semantics. H = row r's history, P = min(|H|, max_pos), t = 0 .. steps-1:
 *   1. Positives of step t: H[(t * max_pos + i) mod |H|], i < P (a rotating window; the whole
 *      history when it fits).
 *   2. Negative (r, t, i, j), j < n_neg: mix(z) is the splitmix64 finaliser (z ^= z >> 30;
 *      z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31);
 *      z0 = mix(seed + 0x9E3779B97F4A7C15 * (r + 1)); for attempt a = 0..7:
 *      x = mix(z0 ^ (t << 40 | i << 24 | j << 8 | a)), c = ((x >> 32) * n_cand) >> 32; the first c with
 *      cand_mask[c] != 0 that is not in H (binary search) is the negative. All eight rejected: the
 *      slot contributes nothing and flag bit 2 is set. Draws depend on r, not on the call's batching.
 *   3. Forward: uf = W2 relu(W1 relu(e) + b1) + b2 (userembedding.py:33-44); cos(uf, f) with both
 *      sides normalised (x / max(||x||, 1e-8)) before the dot product, as the trainer's score;
 *      loss_t = (1/P) sum_i sum_j max(0, margin - (cos(uf, f_pos_i) - cos(uf, f_neg_ij))), the value
 *      BEFORE the step's update, into out_loss[row][t]. An exact tie passes half the gradient.
 *   4. Backward to e only. out_grad (nullable) receives the last executed step's gradient, before
 *      its Adam step.
 *   5. Adam on the row: step count t + 1, scalars formed as dcue_adam_step forms them, constant lr,
 *      moments starting at +0; the trainer's element update (bit-identical to it for the gradient
 *      the kernel produced).
 *   6. out_feat [n_users][d] = tower(final e); with steps == 0 the tower of the initial row.
 *   7. An empty history leaves the row untouched, its losses 0 and sets flag bit 0. A non-finite
 *      loss or factor (or a history entry outside [0, n_cand)) sets bit 1.
 * Workspace: the normalised candidates, the per-step Adam scalars and, for E beyond about 400, the tiles'
 * activations (at most 5 x 16 x (E + 20) floats per 16 users) -- nothing of size n_users x n_cand, no
 * gathered factor rows. dcue_foldin_workspace_bytes is a host computation; dcue_user_foldin
 * validates every argument on the host before its first device call (DCUE_ERR_INVALID: a null
 * required pointer, steps / n_neg / max_pos out of range, n_cand <= 0; DCUE_ERR_UNSUPPORTED:
 * d > 256 or E > 1024; DCUE_ERR_WORKSPACE; n_users == 0 is DCUE_OK) and synchronises `stream`
 * before returning.
 * dcue_foldin_negatives: the sampler alone for `step`, out_neg [n_users][max_pos][n_neg] candidate
 * indices, -1 = a dropped slot or i >= P. Asynchronous on `stream`. */
typedef struct dcue_foldin_config {
  int32_t steps;   /* 0..4096 */
  int32_t n_neg;   /* 1..256 */
  int32_t max_pos; /* 1..1024 */
  float margin;
  double lr, beta1, beta2, eps, weight_decay; /* as dcue_adam_args */
  uint64_t seed;
} dcue_foldin_config;
int dcue_foldin_workspace_bytes(const dcue_dims* dims, int64_t n_cand, int32_t n_users,
                                int32_t max_pos, int32_t n_neg, size_t* bytes_host);
int dcue_user_foldin(const dcue_model* m, const float* cand_feat, int64_t n_cand,
                     const uint8_t* cand_mask, const int64_t* hist_ptr, const int32_t* hist_idx,
                     int32_t n_users, int64_t row0, const dcue_foldin_config* cfg, float* emb,
                     void* ws, size_t ws_bytes, float* out_feat, float* out_loss, float* out_grad,
                     int32_t* out_flags, void* stream);
int dcue_foldin_negatives(int64_t n_cand, const uint8_t* cand_mask, const int64_t* hist_ptr,
                          const int32_t* hist_idx, int32_t n_users, int64_t row0,
                          const dcue_foldin_config* cfg, int32_t step, int32_t* out_neg, void* stream);

/* ------------------------------------------------------- top-K ranking metrics (added under ABI 17) */
/* How good the lists dcue_topk serves are: Precision / Recall / NDCG / MAP / MRR / HitRate at up to
 * DCUE_TOPK_METRICS_MAX_CUTOFFS cutoffs per query, and the exposure counts catalogue coverage is read
 * from, computed on the lists where dcue_topk left them (no list goes to the host, no score matrix).
 * The reference has no counterpart (its only quality numbers are DCUE.score's AUC / mAP).
 *   idx [n_queries][k], count[n_queries]: dcue_topk's out_idx / out_count: list L[0..c), c = count
 *     clamped to 0..k, best first. Entries at j >= c (the -1 padding) are never read.
 *   queries[n_queries]: the query row of each list (repeats allowed; each occurrence counts).
 *   truth_ptr[n_query_rows+1], truth_idx: CSR over query rows of the held-out items T of the query,
 *     t = |T|, each row sorted, no repeats -- dcue_topk's exclusion format.
 *   cutoffs_host[n_cutoffs] (HOST memory): 1 <= k_1 < ... < k_m <= k, 1 <= m <= 8.
 * With h_j = [L[j] in T] for j < c, h_j = 0 for j >= c, and H_j = h_0 + ... + h_j, at a cutoff K:
 *   DCUE_TOPK_METRIC_PRECISION  H_{K-1} / K (K, not min(K, c))
 *   DCUE_TOPK_METRIC_RECALL     H_{K-1} / t
 *   DCUE_TOPK_METRIC_NDCG       (sum_{j<K} h_j / log2(j+2)) / (sum_{j<min(K,t)} 1 / log2(j+2))
 *   DCUE_TOPK_METRIC_MAP        (sum_{j<K} h_j H_j / (j+1)) / min(K, t)
 *   DCUE_TOPK_METRIC_MRR        1 / (j*+1), j* the first j < K with h_j = 1; 0 if there is none
 *   DCUE_TOPK_METRIC_HIT        [H_{K-1} > 0]
 * all in fp64. out_metrics [n_queries][n_cutoffs][DCUE_TOPK_N_METRICS]; a query's numbers are a
 * function of its list and its truth row alone (fixed summation order), so they do not depend on how
 * a caller batches its queries.
 *   out_flags[q] bit 0: the truth row is empty; bit 1: an entry L[j], j < c, lies outside
 *     [0, n_cand) (each entry is range-checked before it addresses anything), or queries[q] lies
 *     outside [0, n_query_rows). A flagged query's metrics are 0, and it is left out of every mean
 *     and of the exposure counts.
 *   exposure (nullable) int32 [n_cutoffs][n_cand]: position j < k_m of an evaluated (unflagged) query
 *     adds 1 to exposure[i][L[j]], i the first cutoff with j < k_i (integer atomics: deterministic).
 *     The kernel accumulates; the caller zeroes the buffer before the first call of an evaluation.
 * dcue_topk_metrics_mean: out_mean [n_cutoffs][DCUE_TOPK_N_METRICS] = the arithmetic mean of `metrics`
 * over the queries with flags == 0, *out_n_evaluated their number (means 0 where it is 0). With
 * `exposure`, out_coverage[i] = (candidates c with exposure[0..i][c] not all zero) / (candidates with a
 * non-zero cand_mask byte; n_cand with a null mask) -- the share of the catalogue that appears in the
 * first k_i entries of at least one evaluated query; out_coverage is null exactly when exposure is.
 * The summation order depends on n_queries and n_cutoffs only (one workgroup, fixed chunks, no
 * floating-point atomics): the means are bit-identical however `metrics` was filled.
 * Both calls validate every argument on the host before their first device call (DCUE_ERR_INVALID: a
 * null required pointer, k outside 1..DCUE_TOPK_MAX_K, n_cutoffs outside 1..8, cutoffs not strictly
 * ascending / below 1 / above k, n_cand <= 0, n_query_rows <= 0, n_queries < 0; DCUE_ERR_UNSUPPORTED:
 * n_cand beyond dcue_topk's bound). n_queries == 0 is DCUE_OK (the means are 0, *out_n_evaluated 0).
 * Both are asynchronous on `stream`. */
#define DCUE_TOPK_METRICS_MAX_CUTOFFS 8
#define DCUE_TOPK_N_METRICS 6
#define DCUE_TOPK_METRIC_PRECISION 0
#define DCUE_TOPK_METRIC_RECALL 1
#define DCUE_TOPK_METRIC_NDCG 2
#define DCUE_TOPK_METRIC_MAP 3
#define DCUE_TOPK_METRIC_MRR 4
#define DCUE_TOPK_METRIC_HIT 5
#define DCUE_TOPK_FLAG_NO_TRUTH 1
#define DCUE_TOPK_FLAG_BAD_INDEX 2
int dcue_topk_metrics(const int32_t* idx, const int32_t* count, int32_t n_queries, int32_t k,
                      const int32_t* queries, const int64_t* truth_ptr, const int32_t* truth_idx,
                      int64_t n_query_rows, int64_t n_cand, const int32_t* cutoffs_host,
                      int32_t n_cutoffs, double* out_metrics, int32_t* out_flags, int32_t* exposure,
                      void* stream);
int dcue_topk_metrics_mean(const double* metrics, const int32_t* flags, int32_t n_queries,
                           int32_t n_cutoffs, const int32_t* exposure, const uint8_t* cand_mask,
                           int64_t n_cand, double* out_mean, double* out_coverage,
                           int32_t* out_n_evaluated, void* stream);

/* ------------------------------------------- diversity-aware serving: MMR, ILD (added under ABI 17) */
/* Maximal Marginal Relevance re-ranking (Carbonell & Goldstein, SIGIR 1998) of the lists dcue_topk /
 * dcue_topk_scored leave on the device, and the intra-list diversity of such lists. The reference has
 * no counterpart.
 * Pool. A list L[0..c) of candidate indices with relevances r[0..c): dcue_topk's out_idx / out_score /
 *   out_count at k = pool, 1 <= pool <= DCUE_TOPK_MAX_K; c = count clamped to 0..pool. Entries at j >= c
 *   are never read. Pool POSITIONS are the entities: a caller-supplied list that names an index twice
 *   has two entries with similarity 1.
 * Similarity. sim(a, b) = the cosine of rows L[a], L[b] of cand_feat [n_cand][d], d <= 256, with the
 *   project's clamp x / max(||x||, 1e-8) on each side, in fp32: (x_a . x_b) * (inv_a * inv_b), inv = 1 /
 *   max(sqrt(x . x), 1e-8), the norms read from the Gram matrix's diagonal. A zero row has similarity 0
 *   to everything. Always the cosine, also for DCUE_SCORE_DOT lists. sim(a, b) and sim(b, a) are the
 *   same bits.
 * Relevance scaling (rel_mode). DCUE_MMR_REL_RAW: r' = r (cosine lists are on the similarity's scale).
 *   DCUE_MMR_REL_MINMAX: r' = (r - min r) / (max r - min r) over the list's c entries, 0 when max == min
 *   (inner-product lists, whose scale is arbitrary); fp32, in exactly this order.
 * Selection. S starts empty; m_a = 0 while S is empty, afterwards m_a = max_{b in S} sim(a, b) (which
 *   may be negative). For t = 0 .. min(k_out, c) - 1 the unselected position a that maximises
 *   f_a = lambda * r'_a - (1 - lambda) * m_a is selected (fp32, every operation rounded on its own);
 *   ties go to the LOWEST pool position -- with dcue_topk's order a total order. 0 <= lambda <= 1;
 *   lambda = 1 returns the first k_out entries of the pool unchanged.
 * Outputs. out_idx [n_lists][k_out], out_score [n_lists][k_out] (the entry's original r, never r' or f),
 *   out_count [n_lists] = min(k_out, c); short lists end in idx -1 / score -inf as dcue_topk's do.
 *   out_flags[i] bit 1 (DCUE_LIST_FLAG_BAD_INDEX): an entry L[j], j < c, lies outside [0, n_cand) --
 *   each entry is range-checked before it addresses anything; bit 2 (DCUE_LIST_FLAG_NONFINITE): a pool
 *   row or a relevance is NaN or infinite (or a row's squared norm overflows fp32). A flagged list gets
 *   count 0 and all padding.
 * ILD. For a list and a cutoff K, n_K = min(K, c):
 *   ILD@K = 2 / (n_K (n_K - 1)) * sum_{a < b < n_K} (1 - sim(a, b)),
 *   fp64 sums over the fp32 similarities in a fixed order (per b ascending a, then ascending b). Where
 *   n_K < 2 the value is 0 and bit 0 (DCUE_LIST_FLAG_NO_PAIR) is set for the list -- so a call whose
 *   cutoffs include 1 flags every list. out_ild [n_lists][n_cutoffs]; bits 1 and 2 as above, all values
 *   0. dcue_list_ild_mean: out_mean[i] = the arithmetic mean of column i over the lists with flags == 0,
 *   *out_n_evaluated their number (means 0 where it is 0); one workgroup, an order that depends on
 *   n_lists and n_cutoffs only: bit-identical however `ild` was filled.
 * Invariance. A list's outputs are a function of that list and the rows it names: they do not depend on
 *   n_lists, on batching, or on which other lists share the launch, bit for bit. The Gram summation
 *   order depends on d alone.
 * cutoffs_host[n_cutoffs] (HOST memory): 1 <= k_1 < ... < k_m <= k, 1 <= m <= 8.
 * The kernels keep a list's rows and its similarity matrix in LDS and need no workspace:
 * dcue_list_mmr_workspace_bytes (a host computation; dcue_list_ild's too, with pool = k) gives 0 today,
 * and ws may then be null; the parameters stay so that this can change without the ABI.
 * All calls are asynchronous on `stream` and validate every argument on the host before their first
 * device call (DCUE_ERR_INVALID: a null required pointer, pool or k outside 1..DCUE_TOPK_MAX_K, k_out
 * outside 1..pool, lambda outside [0, 1] or NaN, an unknown rel_mode, cutoffs not strictly ascending /
 * below 1 / above k, n_cutoffs outside 1..8, n_cand <= 0, d <= 0, n_lists < 0; DCUE_ERR_UNSUPPORTED:
 * d > 256, n_cand beyond dcue_topk's bound; DCUE_ERR_WORKSPACE). n_lists == 0 is DCUE_OK. */
#define DCUE_MMR_REL_RAW 0
#define DCUE_MMR_REL_MINMAX 1
#define DCUE_LIST_FLAG_NO_PAIR 1
#define DCUE_LIST_FLAG_BAD_INDEX 2
#define DCUE_LIST_FLAG_NONFINITE 4
int dcue_list_mmr_workspace_bytes(int32_t pool, int32_t d, int32_t n_lists, size_t* bytes_host);
int dcue_list_mmr(const int32_t* idx, const float* score, const int32_t* count, int32_t n_lists,
                  int32_t pool, const float* cand_feat, int64_t n_cand, int32_t d, float lambda,
                  int32_t rel_mode, int32_t k_out, void* ws, size_t ws_bytes, int32_t* out_idx,
                  float* out_score, int32_t* out_count, int32_t* out_flags, void* stream);
int dcue_list_ild(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                  const float* cand_feat, int64_t n_cand, int32_t d, const int32_t* cutoffs_host,
                  int32_t n_cutoffs, void* ws, size_t ws_bytes, double* out_ild /* [n][m] */,
                  int32_t* out_flags, void* stream);
int dcue_list_ild_mean(const double* ild, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs,
                       double* out_mean /* [m] */, int32_t* out_n_evaluated, void* stream);

/* ------------------------------------------- explained lists: nearest history songs (added under ABI 17) */
/* "Because you played X": for every pick of the lists dcue_topk / dcue_topk_scored / dcue_list_mmr leave
 * on the device, the songs of the user's history most similar to it. The reference has no counterpart.
 * List. idx [n_lists][k] / count [n_lists]: those calls' out_idx / out_count, 1 <= k <= DCUE_TOPK_MAX_K;
 *   list q is L[0..c), c = count clamped to 0..k. Entries at j >= c are never read.
 * History. u = queries[q] is the list's query row; hist_ptr [n_query_rows + 1] / hist_idx is a CSR over
 *   query rows in dcue_topk's exclusion format (candidate indices, each row sorted, no repeats). H_u =
 *   the row's entries h whose byte hist_mask[h] (hist_mask [n_cand], nullable: every entry) is non-zero
 *   -- the mask keeps songs without audio, whose factor rows are zero, out. A row may be any length.
 * Similarity. sim(a, h) = dcue_topk's cosine of rows a and h of cand_feat [n_cand][d], d <= 256, bit for
 *   bit: x / max(||x||, 1e-8) on each side, zero-padded to the next multiple of 16, summed in dcue_topk's
 *   order with row a as the query and row h as the candidate. A reason's similarity is the score an
 *   item-to-item dcue_topk call reports for the pair, whatever else shares the launch.
 * Reasons. For every position j < c, a = L[j]: the members h of H_u whose sim(a, h) is not NaN, by
 *   similarity descending, then candidate index ascending (dcue_topk's total order); the first m go to
 *   out_idx[q][j][0..m) / out_sim[q][j][0..m), 1 <= m <= DCUE_EXPLAIN_MAX_REASONS. Short rows end in
 *   index -1 / similarity -inf; rows j >= c are all padding. A pick that is itself in H_u is kept.
 * Flags. out_flags[q] bit 0 (DCUE_EXPLAIN_FLAG_NO_HISTORY): H_u is empty, the list is all padding. Bit 1
 *   (DCUE_LIST_FLAG_BAD_INDEX): queries[q] lies outside [0, n_query_rows), or an entry L[j], j < c, or an
 *   entry of the history row lies outside [0, n_cand) -- each is range-checked before it addresses
 *   anything, the mask included; the list is all padding and the flags are this bit alone. Bit 2
 *   (DCUE_LIST_FLAG_NONFINITE): a similarity of the list is NaN or infinite; a NaN is never returned,
 *   everything else stands (dcue_topk's rule).
 * Invariance. A list's outputs are a function of the list, its history row and the rows they name: they
 *   do not depend on n_lists, on batching, on which other lists share the launch, or on where the row
 *   sits inside hist_idx, bit for bit.
 * dcue_list_explain_workspace_bytes is a host computation: the workspace holds the candidate table's unit
 * rows, [n_cand][d rounded up to 16] floats. The call is asynchronous on `stream` and validates every
 * argument on the host before its first device call (DCUE_ERR_INVALID: a null required pointer, k
 * outside 1..DCUE_TOPK_MAX_K, m outside 1..DCUE_EXPLAIN_MAX_REASONS, n_cand <= 0, d <= 0, n_query_rows <=
 * 0, n_lists < 0; DCUE_ERR_UNSUPPORTED: d > 256, n_cand beyond dcue_topk's bound; DCUE_ERR_WORKSPACE).
 * n_lists == 0 is DCUE_OK. */
#define DCUE_EXPLAIN_MAX_REASONS 8
#define DCUE_EXPLAIN_FLAG_NO_HISTORY 1 /* bits 1 and 2: DCUE_LIST_FLAG_BAD_INDEX / DCUE_LIST_FLAG_NONFINITE */
int dcue_list_explain_workspace_bytes(int64_t n_cand, int32_t d, int32_t n_lists, int32_t k, int32_t m,
                                      size_t* bytes_host);
int dcue_list_explain(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                      const int32_t* queries, const int64_t* hist_ptr, const int32_t* hist_idx,
                      int64_t n_query_rows, const uint8_t* hist_mask, const float* cand_feat, int64_t n_cand,
                      int32_t d, int32_t m, void* ws, size_t ws_bytes,
                      int32_t* out_idx /* [n_lists][k][m] */, float* out_sim /* [n_lists][k][m] */,
                      int32_t* out_flags /* [n_lists] */, void* stream);

/* ------------------------------------------- audio front end: waveform -> log-mel (added under ABI 17) */
/* The step before the item tower: mono f32 waveforms in, [frame][DCUE_N_MELS] track-table rows out, in
 * one launch -- framing, window, FFT, power, mel filterbank and compression fused; no spectrum goes to
 * HBM and there is no workspace. The reference has no counterpart (its README names a
 * transform_audio.py that was never published), so the definition below is this project's own.
 * Signal. With N = n_fft, pad = N/2 when center = 1 (the clip is reflect-padded: sample -i is sample
 *   i, sample n_samples - 1 + i is sample n_samples - 1 - i) and 0 when center = 0, frame t is samples
 *   [t hop - pad, t hop - pad + N) times the periodic Hann window 0.5 - 0.5 cos(2 pi n / N); a clip has
 *   1 + (n_samples + 2 pad - N) / hop frames (22050 Hz, N 1024, hop 512, center: 66,560 samples give
 *   DCUE_N_FRAMES = 131). S = |rfft|^2, N/2 + 1 bins. Mel bin i of 128 is sum_k w_i[k] S[k]: band edges
 *   f_0..f_129 equally spaced on the Slaney mel scale (linear, 200/3 Hz per mel, below 1 kHz; above,
 *   27 mel per factor 6.4) from fmin to fmax, triangles min((f - f_i) / (f_{i+1} - f_i), (f_{i+2} - f) /
 *   (f_{i+2} - f_{i+1})) clipped at 0, times 2 / (f_{i+2} - f_i) -- librosa's defaults. The sum runs over
 *   the bin's FFT bins in ascending order, always: a row's bits are a function of the frame's samples and
 *   the table alone (not of n_clips, frame0, or what shares the launch).
 * Compression. DCUE_LOGMEL_POWER: P. DCUE_LOGMEL_DB: 10 log10(max(P, amin)) (ref = 1.0); P <= amin gives
 *   the floor 10 log10(amin), rounded once from double. DCUE_LOGMEL_LOG1P: log(1 + log_scale sqrt(P)).
 *   Computed in f32; out_dtype 0 converts to fp16 last (round to nearest even).
 * wave [n_clips][n_samples] f32, already at sample_rate (dcue_resample, below, brings it there). out [n_clips][n_frames][128] of out_dtype: the
 *   dcue_tracks layout, so with n_frames = DCUE_N_FRAMES `out` is a track table as it stands. The call
 *   writes frames frame0 .. frame0 + n_frames - 1 of each clip. flags [n_clips] is zeroed by the call;
 *   bit 0 (DCUE_LOGMEL_FLAG_NONFINITE) is set for a clip when a sample the requested frames read is NaN
 *   or infinite; the other clips' rows are unaffected, bit for bit.
 * Table. dcue_logmel_table_bytes bytes of device memory, filled once per configuration by
 *   dcue_logmel_table_init (which synchronises `stream`): the window, the FFT twiddles, and the filters as
 *   per-bin [first FFT bin, count) runs plus packed weights (a triangle is one contiguous run; a filter
 *   narrower than the FFT's resolution is empty -- count 0 -- and its bin holds the floor: 20 of them at
 *   n_fft 256 and 22050 Hz). dcue_logmel_table_fill_host writes the same bytes to host memory: every
 *   entry computed in double precision and rounded once to f32, so the kernel calls no device
 *   trigonometry. Layout: int32 header[8] {magic, n_fft, n_weights}; f32 window[N]; f32 pairs
 *   exp(-2 pi i t / (N/2)), t < N/2; f32 pairs exp(-2 pi i k / N), k <= N/4; int32 first[128], count[128],
 *   offset[128]; f32 weights[N + 2]. dcue_logmel must be given the table of the same configuration.
 * Every call validates on the host before its first device call, so the refusals below are reachable
 * without a GPU, each with a dcue_last_error text. DCUE_ERR_INVALID: n_fft outside {256, 512, 1024,
 * 2048}; hop < 1 or hop > n_fft; sample_rate < 1; fmin < 0, fmax > sample_rate / 2 or fmin >= fmax; amin
 * <= 0 with DB; an unknown compress / out_dtype / center; center = 1 with n_samples <= n_fft / 2 (the
 * reflection is undefined); center = 0 with n_samples < n_fft; a negative count; a frame range that
 * reaches past the clip's frame count (never padded silently); a null pointer. DCUE_ERR_UNSUPPORTED:
 * n_samples beyond the 32-bit sample index. n_clips == 0 or n_frames == 0 is DCUE_OK. dcue_logmel is
 * asynchronous on `stream`. */
#define DCUE_LOGMEL_POWER 0   /* mel power, no compression (tests, callers with their own log) */
#define DCUE_LOGMEL_DB    1   /* 10*log10(max(P, amin)), ref = 1.0 */
#define DCUE_LOGMEL_LOG1P 2   /* log(1 + log_scale*sqrt(P)) */
#define DCUE_LOGMEL_FLAG_NONFINITE 1
typedef struct dcue_logmel_config {
  int32_t sample_rate, n_fft, hop, center;   /* center: 1 = reflect-pad n_fft/2 each side, 0 = none */
  int32_t compress, out_dtype;               /* out_dtype as dcue_tracks.dtype: 0 fp16, 1 fp32 */
  float fmin, fmax, amin, log_scale;
} dcue_logmel_config;
int dcue_logmel_frames(const dcue_logmel_config* cfg, int64_t n_samples, int64_t* n_frames_host);
int dcue_logmel_table_bytes(const dcue_logmel_config* cfg, size_t* bytes_host);
int dcue_logmel_table_fill_host(const dcue_logmel_config* cfg, void* table_host, size_t bytes);
int dcue_logmel_table_init(const dcue_logmel_config* cfg, void* table_dev, size_t bytes, void* stream);
int dcue_logmel(const dcue_logmel_config* cfg, const void* table_dev, const float* wave, int64_t n_clips,
                int64_t n_samples, int64_t frame0, int32_t n_frames, void* out, int32_t* flags, void* stream);

/* ------------------------------------------- sample-rate conversion ahead of it (added under ABI 17) */
/* Music is distributed at 44.1 or 48 kHz and the model reads 22,050 Hz: dcue_resample converts mono f32
 * waveforms from rate_in to rate_out in one launch, no workspace. The reference has no counterpart; the
 * definition is this project's own, pinned by tests/resample_reference.py.
 * Definition. A rational polyphase resampler with a Kaiser-windowed sinc evaluated exactly per phase (no
 *   interpolated filter table). g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g,
 *   s = rolloff min(1, L / M), Kh = ceil(zeros / s), K = 2 Kh taps per output, n_out = ceil(n_in L / M).
 *   Output m: q = floor(m M / L), p = (m M) mod L,
 *     y[m] = sum_{k=0..K-1} tab[p][k] x[q - Kh + 1 + k],   x = 0 outside [0, n_in),
 *     tab[p][k] = s sinc(u) w(u),  u = s (p / L - (k - Kh + 1)),  sinc(u) = sin(pi u) / (pi u),
 *     w(u) = I0(beta sqrt(1 - (u / zeros)^2)) / I0(beta) for |u| < zeros, 0 otherwise.
 *   Two named qualities carry the published constants of resampy's kaiser_best / kaiser_fast windows:
 *   best = {zeros 64, beta 14.769656459379492, rolloff 0.9475937167399596}, fast = {16, 8.555504641634386,
 *   0.85}; parity with resampy itself (which interpolates a sampled filter) is not claimed.
 * Summation order. y[m] is the chain acc = fmaf(tab[p][k], x[q - Kh + 1 + k], acc) over k = 0 .. K-1 in
 *   ascending order from acc = +0: exact products, one rounding per addition. An output's bits are a
 *   function of its K samples and its phase row alone -- not of n_clips, of out0 / n_out, of the clip's
 *   place in the batch or of what shares the launch.
 * wave [n_clips][n_in] f32. out [n_clips][n_out] f32 holds outputs out0 .. out0 + n_out - 1 of each clip.
 *   There is no flag word: a NaN or infinite sample propagates by IEEE rules into exactly the outputs whose
 *   K samples include it (dcue_logmel's flag then names the clip); other outputs and clips keep their bits.
 * Table. dcue_resample_table_bytes bytes of device memory, filled once per configuration by
 *   dcue_resample_table_init (which synchronises `stream`): int32 header[8] {magic, L, M, K, Kh, zeros,
 *   rate_in, rate_out}, then f32 tab[L][K]. dcue_resample_table_fill_host writes the same bytes to host
 *   memory: every tap computed in double precision (I0 by its power series) and rounded once, so the
 *   kernel calls no device transcendental. dcue_resample must be given the table of the same
 *   configuration; the kernel compares the header with its own L, M, K, Kh and, where they differ, writes
 *   NaN to every output of the call instead of reading taps that are not there.
 * Every call validates on the host before its first device call, so the refusals below are reachable
 * without a GPU, each with a dcue_last_error text. DCUE_ERR_INVALID: a rate < 1; equal rates (nothing to
 * resample); zeros < 1; rolloff outside (0, 1]; beta < 0; a negative count; an output range that reaches
 * past n_out(n_in); a null pointer; a table size other than dcue_resample_table_bytes. DCUE_ERR_UNSUPPORTED:
 * a table larger than DCUE_RESAMPLE_MAX_TABLE_BYTES (32000 -> 22050 `best` is 341 KB; near-coprime rates
 * such as 44100 -> 44101 are refused rather than served slowly); n_in beyond 2^31 - 1; n_clips x output
 * tiles beyond the grid limit. n_clips == 0 or n_out == 0 is DCUE_OK with no launch. dcue_resample is
 * asynchronous on `stream`. */
#define DCUE_RESAMPLE_MAX_TABLE_BYTES (16 << 20)
typedef struct dcue_resample_config {
  int32_t rate_in, rate_out, zeros, reserved;
  double beta, rolloff;
} dcue_resample_config;
int dcue_resample_length(const dcue_resample_config* cfg, int64_t n_in, int64_t* n_out_host);
int dcue_resample_table_bytes(const dcue_resample_config* cfg, size_t* bytes_host);
int dcue_resample_table_fill_host(const dcue_resample_config* cfg, void* table_host, size_t bytes);
int dcue_resample_table_init(const dcue_resample_config* cfg, void* table_dev, size_t bytes, void* stream);
int dcue_resample(const dcue_resample_config* cfg, const void* table_dev, const float* wave,
                  int64_t n_clips, int64_t n_in, int64_t out0, int64_t n_out, float* out, void* stream);

/* ----------------------------------- window crops of full-length tracks (added under ABI 17) */
/* The reference trains on a different DCUE_N_FRAMES-frame window of a song every time it loads the song
 * (DCUEDataset._sample, datasets/dcuedataset.py:166-187: X[:, s:s+131], s = randint(0, T - 131)) and
 * averages its item factors over ten such windows (nn/dcue.py:655-668). dcue_crop_tracks cuts a track
 * table out of full-length tracks kept in HBM, one window per track, by a rule that is a function of
 * (configuration, track index, track length) alone -- not of the output row, the launch or the batch.
 * Store. dcue_track_store: data [total_frames][DCUE_N_MELS], frame-major, fp16 or fp32 -- dcue_tracks'
 *   row layout without the fixed 131 -- and frame_ptr, device int64 [n_tracks + 1]: track t holds frames
 *   frame_ptr[t] .. frame_ptr[t+1] - 1. A track may have length 0 (a song without audio).
 * Output. Row i of out [n_out][131][128] (out_dtype as dcue_tracks.dtype; `out` is a dcue_tracks table as it
 *   stands) is the window of track rows[i] (int32, device), or of track i when rows == NULL. Repeats are
 *   allowed. starts (int32 [n_out], device, nullable) receives the window's first frame inside its track;
 *   flags (int32 [n_out], device) is written for every row: 0, or the bits below.
 * Window rule. L = frame_ptr[t+1] - frame_ptr[t], W = 131, all in 64-bit integers:
 *   L <= W            start 0: the L frames are copied and the other W - L rows are zero (the reference
 *                     pads at the end, F.pad(X, (0, W - L))), whatever the mode.
 *   DCUE_CROP_FIRST   start 0.
 *   DCUE_CROP_CENTER  start (L - W) / 2.
 *   DCUE_CROP_GRID    window grid_j of grid_n evenly spread ones: start grid_j * (L - W) / (grid_n - 1);
 *                     grid_n == 1 is CENTER; grid_j = grid_n - 1 is the last window, start L - W.
 *   DCUE_CROP_RANDOM  start = mulhi64(h, L - W) = floor(h * (L - W) / 2^64), uniform over [0, L - W).
 *                     This is the reference's np.random.randint(0, L - W), whose high end is exclusive: the
 *                     last window (start L - W) is never drawn, and L = W + 1 always gives start 0. That
 *                     is kept. With mix the splitmix64 finaliser of dcue_user_foldin (z ^= z >> 30;
 *                     z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31) and
 *                     G = 0x9E3779B97F4A7C15, all modulo 2^64:
 *                       z0 = mix(seed + G * (t + 1)),  h = mix(z0 + G * (draw + 1)),
 *                     t the track's index in the store. `draw` is the caller's counter (the trainer passes
 *                     its epoch): the same (seed, draw) gives the same table on every rank and in every
 *                     launch; another draw gives every track another, independent window.
 * Conversions. fp16 -> fp32 is exact; fp32 -> fp16 rounds to nearest even, as dcue_logmel does.
 * Guards on the device (frame_ptr and rows are device memory): a row whose extent is negative
 *   (frame_ptr[t] < 0 or frame_ptr[t+1] < frame_ptr[t]) or reaches past total_frames sets
 *   DCUE_CROP_FLAG_BAD_EXTENT; a row whose rows[i] (or i, without rows) lies outside [0, n_tracks) sets
 *   DCUE_CROP_FLAG_BAD_ROW. Such a row is written as zeros with start 0; nothing is read or written out
 *   of bounds and the other rows are unaffected, bit for bit.
 * Refused on the host before any device call, each with a dcue_last_error text (DCUE_ERR_INVALID): a
 *   null store, cfg, out or flags; a negative n_tracks, total_frames or n_out; an unknown mode or dtype;
 *   grid_n < 1, grid_j < 0 or grid_j >= grid_n (GRID); with n_out > 0 a null frame_ptr or data, data or
 *   out not 16-byte aligned, out overlapping the store's data. DCUE_ERR_UNSUPPORTED: total_frames beyond
 *   INT32_MAX (starts are int32). n_out == 0 is DCUE_OK. One launch, no workspace, no LDS; asynchronous
 *   on `stream`.
 * dcue_crop_starts_host: the same arithmetic on the CPU (no device call): starts_host[i] for a track of
 *   lengths_host[i] frames at store index track_ids_host[i] (null: i). For tests, and for callers that
 *   need the windows without reading them back. */
#define DCUE_CROP_FIRST 0
#define DCUE_CROP_CENTER 1
#define DCUE_CROP_GRID 2
#define DCUE_CROP_RANDOM 3
#define DCUE_CROP_FLAG_BAD_EXTENT 1
#define DCUE_CROP_FLAG_BAD_ROW 2
typedef struct dcue_track_store {
  const void* data;         /* [total_frames][128] */
  const int64_t* frame_ptr; /* [n_tracks + 1], device */
  int64_t n_tracks;
  int64_t total_frames;
  int32_t dtype;            /* 0 = fp16, 1 = fp32 */
  int32_t reserved;
} dcue_track_store;
typedef struct dcue_crop_config {
  int32_t mode;             /* DCUE_CROP_* */
  int32_t grid_j, grid_n;   /* DCUE_CROP_GRID */
  int32_t reserved;
  uint64_t seed, draw;      /* DCUE_CROP_RANDOM */
} dcue_crop_config;
int dcue_crop_tracks(const dcue_track_store* store, const dcue_crop_config* cfg, const int32_t* rows,
                     int64_t n_out, void* out, int32_t out_dtype, int32_t* starts, int32_t* flags,
                     void* stream);
int dcue_crop_starts_host(const dcue_crop_config* cfg, const int64_t* lengths_host,
                          const int64_t* track_ids_host, int64_t n, int64_t* starts_host);

/* ----------------------------- augmentation inside the crop launch (added under ABI 17) */
/* dcue_crop_tracks_augmented is dcue_crop_tracks with SpecAugment-style masks (Park et al. 2019), a
 * loudness jitter and a fill, applied while the window is copied: no further pass over the table. Like
 * the window, what a track gets is a function of (configuration, track index, track length) alone --
 * not of the output row, the launch, the batch or the rank.
 * Configuration. dcue_augment_config: 0 <= n_freq, n_time <= DCUE_AUG_MAX_MASKS (4) masks of each kind,
 *   their largest widths 0 <= freq_width (F) <= 128 mel bins and 0 <= time_width (T) <= 131 frames;
 *   gain_db (G) >= 0 and finite, the half-range of the jitter; fill_mode DCUE_AUG_FILL_MEAN or
 *   DCUE_AUG_FILL_CONST with the finite constant fill_value; reserved is zero. The augmentation is off
 *   when n_freq * freq_width == 0, n_time * time_width == 0 and gain_db == 0.
 * Hash streams. h is DCUE_CROP_RANDOM's hash of (seed, draw, t) above, computed whatever cfg->mode is,
 *   and r(i) = mix(h + G64 * (i + 1)) modulo 2^64, mix and G64 = 0x9E3779B97F4A7C15 as above. The gain
 *   uses r(0); frequency mask j uses r(1 + 2j) for its width and r(2 + 2j) for its place; time mask j
 *   uses r(9 + 2j) and r(10 + 2j) -- 9 = 1 + 2 * DCUE_AUG_MAX_MASKS, so the time masks stay where they
 *   are when n_freq changes.
 * Masks. n = min(L, 131) is the number of valid frames of the row.
 *   frequency mask  w = mulhi64(r, F + 1), p = mulhi64(r', 128 - w + 1): mel bins [p, p + w) of every
 *                   valid frame.
 *   time mask       w = min(mulhi64(r, T + 1), n), p = mulhi64(r', n - w + 1): frames [p, p + w).
 *   A row's mask is the union of its masks. The zero tail of a short track is never touched, and a
 *   track with L = 0 stays all zero.
 * Gain. One value g per track, in fp32, every operation rounded to nearest even and none contracted:
 *   u24 = r(0) >> 40, g = gain_db * (float(u24) * 2^-23 - 1.0f) -- the product is the only rounding --
 *   so g lies in [-G, G).
 * Elements. A valid element x (the store's value widened to fp32, which is exact) becomes x + g (one
 *   fp32 add) when it is not masked, and the fill when it is; the result is converted to out_dtype by
 *   the conversion above (exact, or round to nearest even). With gain_db == 0 no add happens: the source
 *   bits go through exactly as in dcue_crop_tracks.
 * Fill. CONST: fill_value; the gain does not apply to it. MEAN: m + g (m when gain_db == 0), m the mean
 *   of the row's n * 128 valid source elements, each first rounded to fp16 (nothing to do for an fp16
 *   store). The sum S is exact integer arithmetic: finite fp16 values are integer multiples of 2^-24
 *   of magnitude at most 65,504, so 16,768 of them, in units of 2^-24, fit an int64; then
 *   m = float32(double(S) * 2^-24 / double(n * 128)), and m is NaN if one of the rounded elements is
 *   not finite. So the fill does not depend on how a row is split into parts, on the reduction tree
 *   or on the launch shape.
 * dcue_crop_tracks_augmented: the arguments of dcue_crop_tracks plus `aug`. With aug == NULL or an aug
 *   that is off it runs dcue_crop_tracks' kernel and gives its bits. Flags, starts and the guards are
 *   dcue_crop_tracks': a flagged row is zeros. Refused on the host before any device call
 *   (DCUE_ERR_INVALID, with a dcue_last_error text): a count or a width out of range, a negative or
 *   non-finite gain_db, a non-finite fill_value, an unknown fill_mode, a non-zero reserved, and
 *   everything dcue_crop_tracks refuses. One launch, no workspace; asynchronous on `stream`.
 * dcue_augment_params_host: the same integer and fp32 arithmetic on the CPU (no device call) for tracks
 *   of lengths_host[i] frames at store indices track_ids_host[i] (null: i): gain_host [n] receives g,
 *   freq_pw_host and time_pw_host (int32 [n][DCUE_AUG_MAX_MASKS][2]) each mask's (place, width), zeros
 *   for the masks past the count. Each of the three may be null. */
#define DCUE_AUG_MAX_MASKS 4
#define DCUE_AUG_FILL_MEAN 0
#define DCUE_AUG_FILL_CONST 1
typedef struct dcue_augment_config {
  int32_t n_freq, freq_width;  /* frequency masks: count, largest width F */
  int32_t n_time, time_width;  /* time masks: count, largest width T */
  float gain_db;               /* G */
  int32_t fill_mode;           /* DCUE_AUG_FILL_* */
  float fill_value;            /* DCUE_AUG_FILL_CONST */
  int32_t reserved;
} dcue_augment_config;
int dcue_crop_tracks_augmented(const dcue_track_store* store, const dcue_crop_config* cfg,
                               const dcue_augment_config* aug, const int32_t* rows, int64_t n_out, void* out,
                               int32_t out_dtype, int32_t* starts, int32_t* flags, void* stream);
int dcue_augment_params_host(const dcue_crop_config* cfg, const dcue_augment_config* aug,
                             const int64_t* lengths_host, const int64_t* track_ids_host, int64_t n,
                             float* gain_host, int32_t* freq_pw_host, int32_t* time_pw_host);

/* ------------------------------ group-aware serving: per-group caps, group statistics (added under ABI 17) */
/* "At most two songs per artist": a cap on how many entries of one group a served list may hold, and the
 * group-level statistics of such lists, on the lists dcue_topk / dcue_topk_scored / dcue_list_mmr leave on
 * the device. A group is whatever the caller's item -> group map says: artist, album, label. The
 * reference has no counterpart.
 * Pool. idx [n_lists][pool] / score [n_lists][pool] / count [n_lists]: those calls' out_idx / out_score /
 *   out_count at k = pool, 1 <= pool <= DCUE_TOPK_MAX_K; c = count clamped to 0..pool. Entries at j >= c
 *   are never read. Pool POSITIONS are the entities, as in dcue_list_mmr: an index named twice is two
 *   entries.
 * Groups. group_of int32 [n_cand] (device): a value in [0, n_groups) is the candidate's group; -1 means
 *   ungrouped -- never capped, and it counts against nothing; any other value sets
 *   DCUE_GROUP_FLAG_BAD_GROUP for the list.
 * Carry (carry_idx, carry_score, carry_count: all null or all given). carry_idx / carry_score
 *   [n_lists][k_out], carry_count [n_lists] clamped to 0..k_out: entries an earlier call already kept for
 *   the list. They go to the output first, unchanged, and count toward their groups. The carry arrays
 *   must not overlap the outputs.
 * Rule. For pool position j < c with group g >= 0, r_j = (carried entries of group g) + (positions i < j
 *   of group g); the position survives iff g < 0 or r_j < cap. The output is the carry followed by the
 *   surviving positions in pool order, truncated to k_out entries, 1 <= k_out <= DCUE_TOPK_MAX_K. r_j
 *   depends on earlier positions' groups, not on earlier decisions, so this equals the sequential greedy
 *   walk that keeps an entry while its group holds fewer than cap kept ones.
 * Outputs. out_idx / out_score [n_lists][k_out]: idx and score bits copied, never recomputed; the tail is
 *   -1 / -inf as dcue_topk pads. out_count [n_lists]: the real entries. out_dropped [n_lists] (nullable):
 *   the pool positions the cap removed before the list filled (the walk stops at k_out entries).
 * Flags. out_flags[i] bit 1 (DCUE_LIST_FLAG_BAD_INDEX): a pool entry j < c or a carried entry lies
 *   outside [0, n_cand) -- each is range-checked before it addresses anything; bit 4
 *   (DCUE_GROUP_FLAG_BAD_GROUP): an in-range entry's group is below -1 or at least n_groups. A list with
 *   either gets count 0, dropped 0 and all padding. Bit 3 (DCUE_GROUP_FLAG_SHORT): out_count < k_out --
 *   the pool ran out under the cap; the entries are valid.
 * Statistics. For a list idx [n_lists][k] / count and a cutoff K, n_K = min(K, c): distinct@K = the
 *   distinct groups among the first n_K positions, every ungrouped position counting as one of its own;
 *   top@K = the most positions one group holds (1 if all are ungrouped and n_K > 0, 0 if n_K = 0).
 *   out_stats int32 [n_lists][n_cutoffs][2] = (distinct, top). Flags: bits 1 and 4 as above; a flagged
 *   list's values are 0 and it adds no exposure. group_exposure (nullable) int32 [n_cutoffs][n_groups]:
 *   position j < c of an unflagged list with group g >= 0 adds 1 to group_exposure[i][g], i the first
 *   cutoff with j < k_i (integer atomics; the kernel accumulates, the caller zeroes).
 *   cutoffs_host[n_cutoffs] (HOST memory): 1 <= k_1 < ... < k_m <= k, 1 <= m <= 8.
 * dcue_list_group_stats_mean: out_mean [n_cutoffs][2] = double(int64 column sum over the lists with flags
 *   == 0) / double(their number), *out_n_evaluated their number (means 0 where it is 0): an exact integer
 *   sum and one division, so the means are the same bits however `stats` was filled. With group_exposure,
 *   out_coverage[i] = (groups with a non-zero exposure in cutoffs 0..i) / (groups with a non-zero byte in
 *   group_present uint8 [n_groups]; n_groups with a null mask), 0 where the denominator is 0;
 *   out_coverage is null exactly when group_exposure is.
 * Invariance. A list's outputs are a function of that list, its carry and the groups they name.
 * One launch per call, no workspace, no floating-point arithmetic on the lists; asynchronous on `stream`.
 * Every argument is validated on the host before the first device call, each refusal with a
 * dcue_last_error text (DCUE_ERR_INVALID: a null required pointer, pool / k / k_out outside
 * 1..DCUE_TOPK_MAX_K, cap < 1, n_groups < 0, n_cand <= 0, n_lists < 0, carry arrays partly given, bad
 * cutoffs, group_exposure without out_coverage or the reverse; DCUE_ERR_UNSUPPORTED: n_cand beyond
 * dcue_topk's bound). n_lists == 0 is DCUE_OK (the mean call then writes zeros). */
#define DCUE_GROUP_FLAG_SHORT 8
#define DCUE_GROUP_FLAG_BAD_GROUP 16
#define DCUE_GROUP_N_STATS 2 /* distinct, top */
int dcue_list_group_cap(const int32_t* idx, const float* score, const int32_t* count, int32_t n_lists, int32_t pool,
                        const int32_t* group_of, int64_t n_cand, int32_t n_groups, int32_t cap, int32_t k_out,
                        const int32_t* carry_idx, const float* carry_score, const int32_t* carry_count,
                        int32_t* out_idx, float* out_score, int32_t* out_count, int32_t* out_dropped,
                        int32_t* out_flags, void* stream);
int dcue_list_group_stats(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                          const int32_t* group_of, int64_t n_cand, int32_t n_groups, const int32_t* cutoffs_host,
                          int32_t n_cutoffs, int32_t* out_stats /* [n][m][2] */, int32_t* out_flags,
                          int32_t* group_exposure, void* stream);
int dcue_list_group_stats_mean(const int32_t* stats, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs,
                               const int32_t* group_exposure, const uint8_t* group_present, int32_t n_groups,
                               double* out_mean /* [m][2] */, double* out_coverage, int32_t* out_n_evaluated,
                               void* stream);

/* ------------------- popularity-bias statistics: novelty, long-tail share, exposure Gini (added under ABI 17) */
/* How far served lists lean on the catalogue's hits, on the lists dcue_topk / dcue_topk_scored /
 * dcue_topk_prior / dcue_list_mmr / dcue_list_group_cap leave on the device. The reference has no
 * counterpart.
 * Item statistics. idx [n_lists][k] / count [n_lists]: those calls' out_idx / out_count, 1 <= k <=
 *   DCUE_TOPK_MAX_K; c = count clamped to 0..k. Entries at j >= c are never read.
 *   item_value double [n_cand] (device; nullable): a per-item number the HOST prepared -- the
 *     self-information -log2 p_i of an item's share of all plays gives novelty. No transcendental runs
 *     on the device. item_tail uint8 [n_cand] (device; nullable): non-zero = a long-tail item. A null
 *     array's column is 0.
 *   For a cutoff K, n_K = min(K, c): value@K = (sum over j < n_K of item_value[L[j]], added in
 *     ascending j in fp64 -- the bits of a sequential loop) / n_K; tail@K = (positions j < n_K with a
 *     non-zero tail byte, an integer count) / n_K, one division.
 *   out_stats double [n_lists][n_cutoffs][2] = (value, tail). cutoffs_host[n_cutoffs] (HOST memory):
 *     1 <= k_1 < ... < k_m <= k, 1 <= m <= 8.
 *   out_flags[i] bit 0: n_K = 0 at some cutoff (an empty list); bit 1 (DCUE_LIST_FLAG_BAD_INDEX): an
 *     entry L[j], j < c, lies outside [0, n_cand) -- each entry is range-checked before it addresses
 *     anything. A flagged list's values are 0 and it is left out of the means.
 * dcue_list_item_stats_mean: out_mean [n_cutoffs][2] = the arithmetic mean over the lists with flags == 0,
 *   *out_n_evaluated their number (means 0 where it is 0), summed in dcue_topk_metrics_mean's fixed order,
 *   which depends on n_lists and n_cutoffs alone.
 * Exposure Gini. exposure int32 [n_cutoffs][n_cand]: dcue_topk_metrics' exposure counts. For cutoff i, over
 *   the n candidates with a non-zero byte in cand_mask (uint8 [n_cand]; null: all n_cand): x_c = the sum
 *   of exposure[i'][c] over i' <= i (the cumulation out_coverage uses), x_(1) <= ... <= x_(n) ascending,
 *     out_gini[i] = double(sum_j (2j - n - 1) x_(j)) / double(n * sum_c x_c),   out_total[i] = sum_c x_c,
 *   and out_gini[i] = 0 where n = 0 or the total is 0. Numerator and denominator are exact integers
 *   (a histogram over the values by integer atomics and one scan), so the result is one fp64 division,
 *   independent of launch shape and arrival order.
 *   Workspace: a 64-byte header and one uint32 histogram bin per value 0..n_lists_max and cutoff;
 *   dcue_exposure_gini_workspace_bytes is a host computation. n_lists_max: the lists that added to
 *   `exposure` (a list names a candidate once, so no count exceeds it). dcue_exposure_gini reads the
 *   number of bins back from ws_bytes: (ws_bytes - 64) / 4 / n_cutoffs. A count outside the histogram
 *   (or a negative one) is never used as an address: that cutoff gets out_total -1 and out_gini 0, and
 *   so does one whose n * total reaches 2^53.
 *   Refused with DCUE_ERR_UNSUPPORTED, on the host: n_cand * n_lists_max * DCUE_TOPK_MAX_K >= 2^53, the
 *   largest n * total lists of at most DCUE_TOPK_MAX_K entries can produce -- n_cand and ws_bytes (the bins
 *   it holds, less one, as n_lists_max) are the arguments the bound is taken from.
 * dcue_list_item_stats* are one launch each, no workspace; dcue_exposure_gini is one memset and two
 * launches. All are asynchronous on `stream`. Every argument is validated on the host before the first
 * device call, each refusal with a dcue_last_error text (DCUE_ERR_INVALID: a null required pointer, k
 * outside 1..DCUE_TOPK_MAX_K, bad cutoffs, n_cutoffs outside 1..8, n_cand <= 0, n_lists < 0, n_lists_max
 * < 0; DCUE_ERR_UNSUPPORTED: n_cand beyond dcue_topk's bound, the 2^53 rule; DCUE_ERR_WORKSPACE: no room
 * for two bins per cutoff). n_lists == 0 is DCUE_OK (the mean call then writes zeros). */
#define DCUE_ITEM_FLAG_EMPTY 1 /* bit 1: DCUE_LIST_FLAG_BAD_INDEX */
#define DCUE_ITEM_N_STATS 2    /* value, tail */
int dcue_list_item_stats(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                         const double* item_value, const uint8_t* item_tail, int64_t n_cand,
                         const int32_t* cutoffs_host, int32_t n_cutoffs, double* out_stats /* [n][m][2] */,
                         int32_t* out_flags, void* stream);
int dcue_list_item_stats_mean(const double* stats, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs,
                              double* out_mean /* [m][2] */, int32_t* out_n_evaluated, void* stream);
int dcue_exposure_gini_workspace_bytes(int64_t n_cand, int32_t n_cutoffs, int64_t n_lists_max, size_t* bytes_host);
int dcue_exposure_gini(const int32_t* exposure, const uint8_t* cand_mask, int64_t n_cand, int32_t n_cutoffs,
                       void* ws, size_t ws_bytes, double* out_gini, int64_t* out_total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCUE_H_ */
