"""ctypes binding of libdcue_hip.so (include/dcue.h) -- the only way this package computes.

There is no CPU or eager-PyTorch fallback: if the library is missing or a call fails, this module
raises. PyTorch is used for device memory (the caching allocator owns every buffer) and for the
current HIP stream, nothing else.
"""
import ctypes
import os

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("DCUE_HIP_LIB", os.path.join(_PKG_ROOT, "lib", "libdcue_hip.so"))

N_MELS = 128
N_FRAMES = 131
N_BN = 6
N_DENSE_SEGMENTS = 30
SEG_LATE = 6  # DCUE_SEG_LATE: bn0, conv layer 1, bn1 come first in the flat layout
ERR_UNSUPPORTED = 2
LAYOUT_CATALOGUE = 0
LAYOUT_GATHER = 1

STATUS = {0: "DCUE_OK", 1: "DCUE_ERR_INVALID", 2: "DCUE_ERR_UNSUPPORTED", 3: "DCUE_ERR_HIP",
          4: "DCUE_ERR_WORKSPACE"}

# reference parameter names of the flat dense buffer, in segment order (capi.hip param_sizes)
DENSE_NAMES = (["conv.bn0.weight", "conv.bn0.bias"]
               + [n for l in range(1, 6) for n in ("conv.layer%d.weight" % l, "conv.layer%d.bias" % l,
                                                   "conv.bn%d.weight" % l, "conv.bn%d.bias" % l)]
               + ["conv.fc.weight", "conv.fc.bias", "user_embd.linear1.weight",
                  "user_embd.linear1.bias", "user_embd.linear2.weight", "user_embd.linear2.bias"]
               # the mixed audio + text tower's text conv (BASELINE config 4; empty segments otherwise)
               + ["text.conv.weight", "text.conv.bias"])


class Dims(ctypes.Structure):
    _fields_ = [("conv_hidden", ctypes.c_int32), ("feature_dim", ctypes.c_int32),
                ("user_embdim", ctypes.c_int32), ("tower", ctypes.c_int32),
                ("n_users", ctypes.c_int64), ("text_dim", ctypes.c_int32), ("word_dim", ctypes.c_int32),
                ("text_len", ctypes.c_int32), ("text_pad", ctypes.c_int32)]


class Model(ctypes.Structure):
    _fields_ = [("dims", Dims)] + [(n, ctypes.c_void_p) for n in (
        "params", "grads", "exp_avg", "exp_avg_sq", "emb", "emb_exp_avg", "emb_exp_avg_sq",
        "emb_grad", "emb_slot", "bn_stats", "bn_batches", "wpack", "emb_rows", "emb_step", "emb_log")] + [
        ("emb_log_cap", ctypes.c_int32), ("reserved", ctypes.c_int32), ("words", ctypes.c_void_p),
        ("n_words", ctypes.c_int64), ("words_exp", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


class Batch(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int32), ("n_neg", ctypes.c_int32), ("n_items", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("users", ctypes.c_void_p),
                ("item_track", ctypes.c_void_p), ("neg_item", ctypes.c_void_p)]


class Tracks(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("n_tracks", ctypes.c_int64), ("dtype", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("tokens", ctypes.c_void_p)]


class AdamArgs(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("step", ctypes.c_int32),
                ("parts", ctypes.c_int32), ("grad_div", ctypes.c_double)]


class OptArgs(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("step", ctypes.c_int32), ("lr", ctypes.c_double),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("alpha", ctypes.c_double), ("k", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("n_sma_threshold", ctypes.c_double), ("grad_div", ctypes.c_double)]


class OptState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("dense_a", "dense_b", "dense_c", "emb_a", "emb_b", "emb_c")]


OPT_SGD = 1
OPT_RANGER = 2

ADAM_DENSE = 1
ADAM_EMBEDDING = 2

PLAN_SAMPLE_INBATCH = 1
PLAN_GRAPH = 2

TIMED_CONV1_WGRAD = 0
TIMED_CONV1_FWD = 1
TIMED_EMB_FLUSH = 2
TIMED_ADAM_EMBED = 3
TIMED_ALLREDUCE = 4
TIMED_EMB_SLICE = 5
TIMED_TEXT_FWD = 6
TIMED_USER_FWD = 7
TIMED_TEXT_WGRAD = 8
COMM_ID_BYTES = 128


class PlanConfig(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_int32), ("margin", ctypes.c_float), ("emb_grad_scale", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("mt", ctypes.c_void_p)]


class FoldinConfig(ctypes.Structure):
    """dcue_foldin_config (fold-in of unseen users, added under ABI 17)."""
    _fields_ = [("steps", ctypes.c_int32), ("n_neg", ctypes.c_int32), ("max_pos", ctypes.c_int32),
                ("margin", ctypes.c_float), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("seed", ctypes.c_uint64)]


class LogmelConfig(ctypes.Structure):
    """dcue_logmel_config (the audio front end, added under ABI 17)."""
    _fields_ = [("sample_rate", ctypes.c_int32), ("n_fft", ctypes.c_int32), ("hop", ctypes.c_int32),
                ("center", ctypes.c_int32), ("compress", ctypes.c_int32), ("out_dtype", ctypes.c_int32),
                ("fmin", ctypes.c_float), ("fmax", ctypes.c_float), ("amin", ctypes.c_float),
                ("log_scale", ctypes.c_float)]


class ResampleConfig(ctypes.Structure):
    """dcue_resample_config (sample-rate conversion, added under ABI 17)."""
    _fields_ = [("rate_in", ctypes.c_int32), ("rate_out", ctypes.c_int32), ("zeros", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("beta", ctypes.c_double), ("rolloff", ctypes.c_double)]


class TrackStore(ctypes.Structure):
    """dcue_track_store (full-length tracks for dcue_crop_tracks, added under ABI 17)."""
    _fields_ = [("data", ctypes.c_void_p), ("frame_ptr", ctypes.c_void_p), ("n_tracks", ctypes.c_int64),
                ("total_frames", ctypes.c_int64), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CropConfig(ctypes.Structure):
    """dcue_crop_config."""
    _fields_ = [("mode", ctypes.c_int32), ("grid_j", ctypes.c_int32), ("grid_n", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64), ("draw", ctypes.c_uint64)]


class AugmentConfig(ctypes.Structure):
    """dcue_augment_config (augmentation inside the crop launch, added under ABI 17)."""
    _fields_ = [("n_freq", ctypes.c_int32), ("freq_width", ctypes.c_int32), ("n_time", ctypes.c_int32),
                ("time_width", ctypes.c_int32), ("gain_db", ctypes.c_float), ("fill_mode", ctypes.c_int32),
                ("fill_value", ctypes.c_float), ("reserved", ctypes.c_int32)]


class WeightTables(ctypes.Structure):
    """dcue_weight_tables (dcue_sample_catalogue_weighted, added under ABI 17): device uint32 arrays."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("cum", "user_key", "user_skip", "user_weight")]


CROP_FIRST, CROP_CENTER, CROP_GRID, CROP_RANDOM = 0, 1, 2, 3  # DCUE_CROP_*
CROP_FLAG_BAD_EXTENT, CROP_FLAG_BAD_ROW = 1, 2
CROP_FACTOR_DRAW0 = 1 << 32  # the item-factor passes' draws: 2^32 + j, apart from every epoch's
AUG_MAX_MASKS = 4  # DCUE_AUG_MAX_MASKS
AUG_FILL_MEAN, AUG_FILL_CONST = 0, 1  # DCUE_AUG_FILL_*
LOGMEL_POWER, LOGMEL_DB, LOGMEL_LOG1P = 0, 1, 2  # DCUE_LOGMEL_*
LOGMEL_MODES = {"power": LOGMEL_POWER, "db": LOGMEL_DB, "log1p": LOGMEL_LOG1P}
LOGMEL_FLAG_NONFINITE = 1
LOGMEL_N_FFT = (256, 512, 1024, 2048)
# (zeros, beta, rolloff): the published constants of resampy's kaiser_best / kaiser_fast windows
RESAMPLE_QUALITIES = {"best": (64, 14.769656459379492, 0.9475937167399596), "fast": (16, 8.555504641634386, 0.85)}
RESAMPLE_MAX_TABLE_BYTES = 16 << 20  # DCUE_RESAMPLE_MAX_TABLE_BYTES
FOLDIN_MAX_STEPS, FOLDIN_MAX_NEG, FOLDIN_MAX_POS = 4096, 256, 1024
FOLDIN_EMPTY, FOLDIN_NONFINITE, FOLDIN_DROPPED = 1, 2, 4  # out_flags bits
# dcue_select_negatives (hard negatives, added under ABI 17): DCUE_SELECT_MAX_POOL, DCUE_SELECT_FLAG_*
SELECT_MAX_POOL = 1024
SELECT_FLAG_NONFINITE, SELECT_FLAG_BAD_ID = 1, 2
MT_STATE_BYTES = 624 * 4 + 16
MAX_LOG_CAP = 256
ABI_VERSION = 17
COMM_F32, COMM_U64 = 0, 1  # dcue_host_allreduce_fn dtypes
HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32)
RANK_SPLIT, RANK_SINGLE = 0, 1
TOPK_MAX_K = 128  # DCUE_TOPK_MAX_K
SCORE_COSINE, SCORE_DOT = 0, 1  # dcue_topk_scored (added under ABI 17): DCUE_SCORE_*
SCORES = {"cosine": SCORE_COSINE, "dot": SCORE_DOT}
# dcue_topk_metrics (added under ABI 17): cutoffs per call, metrics per cutoff and their slots, flag bits
TOPK_METRICS_MAX_CUTOFFS = 8
TOPK_N_METRICS = 6
TOPK_METRIC_NAMES = ("precision", "recall", "ndcg", "map", "mrr", "hit")  # DCUE_TOPK_METRIC_* order
TOPK_FLAG_NO_TRUTH, TOPK_FLAG_BAD_INDEX = 1, 2
# dcue_list_mmr / dcue_list_ild (added under ABI 17): DCUE_MMR_REL_*, DCUE_LIST_FLAG_*
MMR_REL_RAW, MMR_REL_MINMAX = 0, 1
MMR_RELS = {"raw": MMR_REL_RAW, "minmax": MMR_REL_MINMAX}
LIST_FLAG_NO_PAIR, LIST_FLAG_BAD_INDEX, LIST_FLAG_NONFINITE = 1, 2, 4
# dcue_list_explain (added under ABI 17): DCUE_EXPLAIN_MAX_REASONS, DCUE_EXPLAIN_FLAG_NO_HISTORY (bits 1 and 2:
# LIST_FLAG_BAD_INDEX / LIST_FLAG_NONFINITE)
EXPLAIN_MAX_REASONS = 8
EXPLAIN_FLAG_NO_HISTORY = 1
# dcue_list_group_cap / dcue_list_group_stats (added under ABI 17): DCUE_GROUP_FLAG_*, DCUE_GROUP_N_STATS (bit 1:
# LIST_FLAG_BAD_INDEX)
GROUP_FLAG_SHORT, GROUP_FLAG_BAD_GROUP = 8, 16
GROUP_N_STATS = 2  # distinct, top
# dcue_list_item_stats / dcue_exposure_gini (added under ABI 17): DCUE_ITEM_FLAG_EMPTY, DCUE_ITEM_N_STATS (bit 1:
# LIST_FLAG_BAD_INDEX)
ITEM_FLAG_EMPTY = 1
ITEM_N_STATS = 2  # value (novelty), tail
# dcue_debug_delay sites (include/dcue.h)
DEBUG_SITES = ("user_fwd", "user_bwd", "wgrad_hi", "wgrad_2", "fc_wgrad", "late_adam", "prologue", "lookahead",
               "conv2", "dgrad_2", "wgrad_1", "text_fwd", "dgrad_4", "dgrad_3")

_P = ctypes.c_void_p
_SIGS = {
    "dcue_abi_version": ([], ctypes.c_int),
    "dcue_launch_count": ([], ctypes.c_int64),
    "dcue_last_error": ([], ctypes.c_char_p),
    "dcue_storage_dims": ([ctypes.POINTER(Dims), ctypes.POINTER(Dims)], ctypes.c_int),
    "dcue_param_layout": ([ctypes.POINTER(Dims), _P], ctypes.c_int),
    "dcue_bn_layout": ([ctypes.POINTER(Dims), _P], ctypes.c_int),
    "dcue_wpack_floats": ([ctypes.POINTER(Dims), _P], ctypes.c_int),
    "dcue_workspace_bytes": ([ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                              ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_workspace_outputs": ([ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_workspace_activations": ([ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_workspace_text": ([ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                             ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_debug_text_shape": ([ctypes.POINTER(Dims), ctypes.c_int32, _P, ctypes.c_int32], ctypes.c_int),
    "dcue_pack_weights": ([ctypes.POINTER(Model), _P], ctypes.c_int),
    "dcue_forward": ([ctypes.POINTER(Model), ctypes.POINTER(Batch), ctypes.POINTER(Tracks), _P,
                      ctypes.c_size_t, ctypes.c_int32, ctypes.c_float, _P, _P, _P, _P, _P], ctypes.c_int),
    "dcue_train_backward": ([ctypes.POINTER(Model), ctypes.POINTER(Batch), ctypes.POINTER(Tracks), _P,
                             ctypes.c_size_t, _P, ctypes.c_float, _P], ctypes.c_int),
    "dcue_wrmf_workspace_bytes": ([ctypes.c_int32, ctypes.c_int64, _P], ctypes.c_int),
    "dcue_wrmf_half_step": ([_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, ctypes.c_float,
                             ctypes.c_float, _P, ctypes.c_size_t, _P], ctypes.c_int),
    "dcue_dcbr_step": ([ctypes.POINTER(Model), ctypes.POINTER(Batch), ctypes.POINTER(Tracks), _P, _P, _P,
                        ctypes.c_size_t, _P], ctypes.c_int),
    "dcue_adam_step": ([ctypes.POINTER(Model), ctypes.POINTER(AdamArgs), _P], ctypes.c_int),
    "dcue_optimizer_step": ([ctypes.POINTER(Model), ctypes.POINTER(OptArgs), ctypes.POINTER(OptState), _P],
                            ctypes.c_int),
    "dcue_item_tower_eval": ([ctypes.POINTER(Model), ctypes.POINTER(Tracks), _P, ctypes.c_int32, _P,
                              ctypes.c_size_t, _P, _P], ctypes.c_int),
    "dcue_user_tower": ([ctypes.POINTER(Model), _P, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P],
                        ctypes.c_int),
    "dcue_transpose_spectrograms": ([_P, ctypes.c_int32, _P, _P], ctypes.c_int),
    "dcue_mt_seed": ([_P, ctypes.c_uint32, _P], ctypes.c_int),
    "dcue_mt_draw": ([_P, _P, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_sample_inbatch": ([_P, ctypes.c_int32, ctypes.c_int32, _P, _P], ctypes.c_int),
    "dcue_sample_catalogue": ([_P, ctypes.c_int32, ctypes.c_uint32, _P, ctypes.c_int64, _P, _P, _P,
                               ctypes.c_int32, ctypes.c_int32, _P, _P], ctypes.c_int),
    "dcue_sample_catalogue_weighted": ([_P, ctypes.c_int32, ctypes.c_uint32, _P, ctypes.c_int64, _P, _P,
                                        ctypes.POINTER(WeightTables), _P, ctypes.c_int32, ctypes.c_int32, _P, _P],
                                       ctypes.c_int),
    "dcue_select_negatives": ([_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, _P, ctypes.c_int32,
                               ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "dcue_build_catalogue_batch": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P], ctypes.c_int),
    "dcue_emb_log_bytes": ([ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_emb_log_init": ([ctypes.POINTER(Model), ctypes.c_int32, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_embedding_sync": ([ctypes.POINTER(Model), _P, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_embedding_flush": ([ctypes.POINTER(Model), _P], ctypes.c_int),
    "dcue_plan_create": ([ctypes.POINTER(Model), ctypes.POINTER(Batch), ctypes.POINTER(Tracks), _P, ctypes.c_size_t,
                          ctypes.POINTER(PlanConfig), ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "dcue_plan_launch": ([_P, _P, _P, _P], ctypes.c_int),
    "dcue_plan_destroy": ([_P], ctypes.c_int),
    "dcue_plan_step": ([_P, _P, _P, ctypes.POINTER(AdamArgs), _P], ctypes.c_int),
    "dcue_plan_wait_side": ([_P, _P], ctypes.c_int),
    "dcue_plan_sync": ([_P, _P], ctypes.c_int),
    "dcue_plan_set_next": ([_P, _P], ctypes.c_int),
    "dcue_check_finite": ([_P, ctypes.c_int64, _P, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_check_ids": ([_P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_comm_unique_id": ([_P], ctypes.c_int),
    "dcue_comm_create": ([_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "dcue_comm_create_host": ([ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.POINTER(ctypes.c_void_p)],
                              ctypes.c_int),
    "dcue_comm_destroy": ([_P], ctypes.c_int),
    "dcue_comm_allreduce_mean": ([_P, _P, ctypes.c_int64, _P], ctypes.c_int),
    "dcue_comm_allgather": ([_P, _P, ctypes.c_int64, _P], ctypes.c_int),
    "dcue_plan_set_comm": ([_P, _P], ctypes.c_int),
    "dcue_plan_set_sync_bn": ([_P, ctypes.c_int32], ctypes.c_int),
    "dcue_timer_enable": ([ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
    "dcue_timer_read": ([ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)],
                        ctypes.c_int),
    "dcue_timer_samples": ([ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.c_int64,
                            ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "dcue_rank_workspace_bytes": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_rank_metrics": ([_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32, _P, _P,
                           _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P, _P], ctypes.c_int),
    "dcue_topk_workspace_bytes": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_topk": ([_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32, _P, _P, _P,
                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P, _P, _P],
                  ctypes.c_int),
    "dcue_topk_scored": ([ctypes.c_int32, _P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32,
                          _P, _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P,
                          _P, _P], ctypes.c_int),
    "dcue_topk_prior": ([ctypes.c_int32, _P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32,
                         _P, _P, _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P,
                         _P, _P, _P], ctypes.c_int),
    "dcue_wrmf_objective_workspace_bytes": ([ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_wrmf_objective": ([_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, ctypes.c_double,
                             ctypes.c_double, _P, ctypes.c_size_t, _P, _P], ctypes.c_int),
    "dcue_topk_metrics": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, _P,
                           ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "dcue_topk_metrics_mean": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, _P, _P, _P],
                               ctypes.c_int),
    "dcue_list_mmr_workspace_bytes": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_list_mmr": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                       ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P, _P, _P], ctypes.c_int),
    "dcue_list_ild": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32,
                       _P, ctypes.c_size_t, _P, _P, _P], ctypes.c_int),
    "dcue_list_ild_mean": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P], ctypes.c_int),
    "dcue_list_explain_workspace_bytes": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_list_explain": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64,
                           ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P, _P], ctypes.c_int),
    "dcue_list_group_cap": ([_P, _P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int32,
                             ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "dcue_list_group_stats": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int64, ctypes.c_int32, _P,
                               ctypes.c_int32, _P, _P, _P, _P], ctypes.c_int),
    "dcue_list_group_stats_mean": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_int32, _P, _P, _P, _P],
                                   ctypes.c_int),
    "dcue_list_item_stats": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, ctypes.c_int32, _P,
                              _P, _P], ctypes.c_int),
    "dcue_list_item_stats_mean": ([_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P], ctypes.c_int),
    "dcue_exposure_gini_workspace_bytes": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                            ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_exposure_gini": ([_P, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P, _P], ctypes.c_int),
    "dcue_factor_repeat_mean": ([_P, ctypes.c_int64, ctypes.c_int32, _P], ctypes.c_int),
    "dcue_foldin_workspace_bytes": ([ctypes.POINTER(Dims), ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_user_foldin": ([ctypes.POINTER(Model), _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int32, ctypes.c_int64,
                          ctypes.POINTER(FoldinConfig), _P, _P, ctypes.c_size_t, _P, _P, _P, _P, _P], ctypes.c_int),
    "dcue_foldin_negatives": ([ctypes.c_int64, _P, _P, _P, ctypes.c_int32, ctypes.c_int64,
                               ctypes.POINTER(FoldinConfig), ctypes.c_int32, _P, _P], ctypes.c_int),
    "dcue_logmel_frames": ([ctypes.POINTER(LogmelConfig), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
                           ctypes.c_int),
    "dcue_logmel_table_bytes": ([ctypes.POINTER(LogmelConfig), ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_logmel_table_fill_host": ([ctypes.POINTER(LogmelConfig), _P, ctypes.c_size_t], ctypes.c_int),
    "dcue_logmel_table_init": ([ctypes.POINTER(LogmelConfig), _P, ctypes.c_size_t, _P], ctypes.c_int),
    "dcue_logmel": ([ctypes.POINTER(LogmelConfig), _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                     ctypes.c_int32, _P, _P, _P], ctypes.c_int),
    "dcue_resample_length": ([ctypes.POINTER(ResampleConfig), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
                             ctypes.c_int),
    "dcue_resample_table_bytes": ([ctypes.POINTER(ResampleConfig), ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dcue_resample_table_fill_host": ([ctypes.POINTER(ResampleConfig), _P, ctypes.c_size_t], ctypes.c_int),
    "dcue_resample_table_init": ([ctypes.POINTER(ResampleConfig), _P, ctypes.c_size_t, _P], ctypes.c_int),
    "dcue_resample": ([ctypes.POINTER(ResampleConfig), _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                       ctypes.c_int64, _P, _P], ctypes.c_int),
    "dcue_crop_tracks": ([ctypes.POINTER(TrackStore), ctypes.POINTER(CropConfig), _P, ctypes.c_int64, _P,
                          ctypes.c_int32, _P, _P, _P], ctypes.c_int),
    "dcue_crop_starts_host": ([ctypes.POINTER(CropConfig), _P, _P, ctypes.c_int64, _P], ctypes.c_int),
    "dcue_crop_tracks_augmented": ([ctypes.POINTER(TrackStore), ctypes.POINTER(CropConfig),
                                    ctypes.POINTER(AugmentConfig), _P, ctypes.c_int64, _P, ctypes.c_int32, _P, _P, _P],
                                   ctypes.c_int),
    "dcue_augment_params_host": ([ctypes.POINTER(CropConfig), ctypes.POINTER(AugmentConfig), _P, _P, ctypes.c_int64,
                                  _P, _P, _P], ctypes.c_int),
    "dcue_debug_delay": ([ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
    "dcue_debug_probes": ([_P], ctypes.c_int),
    "dcue_debug_probe_count": ([], ctypes.c_int),
    "dcue_debug_probe_name": ([ctypes.c_int32], ctypes.c_char_p),
    "dcue_debug_poison": ([ctypes.c_int32], ctypes.c_int),
    "dcue_debug_fail_flags": ([_P], ctypes.c_int),
    "dcue_debug_raise_fail_flags": ([ctypes.c_uint32], ctypes.c_int),
    "dcue_debug_launch_shape": ([ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.c_int32, _P, ctypes.c_int32], ctypes.c_int),
}

_lib = None


def poison_on():
    """DCUE_POISON=1 (debug): every workspace the library is handed, and the scratch plans allocate,
    starts as 0xFF bytes (float NaN), so a read of a word no kernel wrote shows as a non-finite result."""
    return os.environ.get("DCUE_POISON", "0") == "1"


def lib():
    """Load libdcue_hip.so (raises if absent: the HIP path is the only path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libdcue_hip.so not found at %s -- build it with `make -C "
                               "amplifai-deepcontentrecommenders_amd` (no CPU fallback exists)" % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = res
        if handle.dcue_abi_version() != ABI_VERSION:
            raise RuntimeError("libdcue_hip ABI mismatch")
        if poison_on():  # debug: plan scratch starts as NaN bytes (dcue_debug_poison)
            handle.dcue_debug_poison(1)
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = "%s failed: %s" % (what, STATUS.get(status, status))
        # the calls that leave a dcue_last_error text
        if status == 3 or what.startswith(("dcue_logmel", "dcue_crop", "dcue_augment", "dcue_resample",
                                         "dcue_list_group", "dcue_topk_prior", "dcue_list_item",
                                         "dcue_exposure_gini")):
            msg += " [%s]" % lib().dcue_last_error().decode(errors="replace")
        raise RuntimeError(msg)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_handle(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be a GPU tensor (the DCUE path runs only on the MI355X)" % name)


TOWERS = {"truedcuemel1dbn": 0, "truedcuemel1d": 1, "truedcuemel1dres": 2, "truedcuemel1dresbn": 3,
          "truedcuemel1dbntext": 4}
TEXT_TOWER = "truedcuemel1dbntext"


def make_dims(conv_hidden, feature_dim, user_embdim, n_users, model_type="truedcuemel1dbn", text=None):
    """text = (text_dim, word_dim, text_len, pad_idx) for the text tower (BASELINE config 4)."""
    t = tuple(text) if model_type == TEXT_TOWER else (0, 0, 0, 0)
    return Dims(conv_hidden, feature_dim, user_embdim, TOWERS[model_type], n_users, *t)


def text_storage(text_dim):
    """The text branch's storage channels (64, 128 or 256: text.hip's column tiles)."""
    return 64 if text_dim <= 64 else 128 if text_dim <= 128 else 256


def words_exponent(words):
    """dcue_model.words_exp: the power of two that puts max |word value| in [2^13, 2^15) before the
    kernels' fp16 hi/lo split (include/dcue.h)."""
    import math
    m = float(words.detach().abs().max()) if words.numel() else 0.0
    if not m > 0.0 or not math.isfinite(m):
        return 0
    return max(-60, min(60, 14 - math.frexp(m)[1]))


def storage_dims(dims):
    """The widths the library stores and computes at (H, d rounded up to 32/64/128/256)."""
    out = Dims()
    check(lib().dcue_storage_dims(ctypes.byref(dims), ctypes.byref(out)), "dcue_storage_dims")
    return out


def segment_shapes(dims):
    """Storage shape of each dense segment (DENSE_NAMES order) for the storage widths of `dims`;
    the reference-shaped parameter is the leading corner of it (include/dcue.h, dcue_storage_dims)."""
    sd = storage_dims(dims)
    Hs, Ds, E, H = sd.conv_hidden, sd.feature_dim, sd.user_embdim, dims.conv_hidden
    res = dims.tower in (TOWERS["truedcuemel1dres"], TOWERS["truedcuemel1dresbn"])
    text = dims.tower == TOWERS[TEXT_TOWER]
    CTs = text_storage(dims.text_dim) if text else 0
    cin = [N_MELS, Hs, Hs, Hs, Hs]
    cout = [Hs, Hs, Hs, Hs, Ds]
    ks = [4, 4, 4, 2, 1]
    shapes = [(N_MELS,), (N_MELS,)]
    for l in range(5):
        shapes += [(cout[l], cin[l], ks[l]), (cout[l],), (cout[l],), (cout[l],)]
    fi = 4 * H + Ds if res else dims.text_dim + Ds if text else Ds
    shapes += [(Ds, fi), (Ds,), (E, E), (E,), (Ds, E), (Ds,)]
    shapes += [(CTs, dims.word_dim if text else 0, 3), (CTs,)]
    return shapes


def corner(buf, off, storage_shape, shape):
    """View of the reference-shaped corner `shape` of the segment at `off` with `storage_shape`."""
    n = 1
    for v in storage_shape:
        n *= v
    seg = buf[off:off + n].view(storage_shape)
    return seg[tuple(slice(0, v) for v in shape)]


def param_layout(dims):
    off = (ctypes.c_int64 * (N_DENSE_SEGMENTS + 1))()
    check(lib().dcue_param_layout(ctypes.byref(dims), ctypes.cast(off, _P)), "dcue_param_layout")
    return list(off)


def bn_layout(dims):
    off = (ctypes.c_int64 * (2 * N_BN + 1))()
    check(lib().dcue_bn_layout(ctypes.byref(dims), ctypes.cast(off, _P)), "dcue_bn_layout")
    return list(off)


def wpack_floats(dims):
    n = ctypes.c_int64()
    check(lib().dcue_wpack_floats(ctypes.byref(dims), ctypes.cast(ctypes.byref(n), _P)), "dcue_wpack_floats")
    return n.value


def workspace_outputs(dims, B, N, M):
    """Byte offsets of (scores, user feats, item feats, loss) inside a (B, N, M) workspace."""
    off = (ctypes.c_size_t * 4)()
    check(lib().dcue_workspace_outputs(ctypes.byref(dims), B, N, M, off), "dcue_workspace_outputs")
    return list(off)


def workspace_activations(dims, B, N, M):
    """Byte offsets of (y_l, argmax_l) for conv layers l = 1..5 inside a (B, N, M) workspace."""
    off = (ctypes.c_size_t * 10)()
    check(lib().dcue_workspace_activations(ctypes.byref(dims), B, N, M, off), "dcue_workspace_activations")
    return [(off[2 * i], off[2 * i + 1]) for i in range(5)]


def timer_enable(kernel, enable=True):
    """enable: True / 1 times every launch of the class, n > 1 every n-th, False / 0 none."""
    check(lib().dcue_timer_enable(kernel, int(enable)), "dcue_timer_enable")


def timer_samples(kernel, cap=4096):
    """Each recorded launch's duration in ms (the first `cap`) since the last read (waits; resets)."""
    buf = (ctypes.c_float * cap)()
    n = ctypes.c_int64()
    check(lib().dcue_timer_samples(kernel, buf, cap, ctypes.byref(n)), "dcue_timer_samples")
    return [float(buf[i]) for i in range(min(n.value, cap))]


def timer_read(kernel):
    """(total ms, launches) of the kernel class since the last read (waits for the events)."""
    ms, n = ctypes.c_double(), ctypes.c_int64()
    check(lib().dcue_timer_read(kernel, ctypes.byref(ms), ctypes.byref(n)), "dcue_timer_read")
    return ms.value, n.value


def emb_log_bytes(cap):
    n = ctypes.c_size_t()
    check(lib().dcue_emb_log_bytes(cap, ctypes.byref(n)), "dcue_emb_log_bytes")
    return n.value


def workspace_bytes(dims, max_rows, max_neg, max_items):
    n = ctypes.c_size_t()
    check(lib().dcue_workspace_bytes(ctypes.byref(dims), max_rows, max_neg, max_items, ctypes.byref(n)),
          "dcue_workspace_bytes")
    return n.value


LAUNCH_SHAPE_WORDS = 74  # DCUE_LAUNCH_SHAPE_WORDS
WGRAD_KERNELS = {0: "wgrad16t", 3: "conv1_wgrad", 4: "multi_f16", 5: "multi_f32"}  # by WK_* code


def launch_shape(dims, layout, B, N, M):
    """The kernel variants a training step of this shape launches (dcue_debug_launch_shape; host
    only, no GPU needed), as a dict: "fwd" {layer: (TW, DEEP, f16, last_rows, spans_items)} for conv
    1..5, "dgrad" the same for layers 2..5, "wgrad" {layer: (kernel, nchunk, rows_per_chunk,
    last_chunk_rows)} for layers 1..6 (kernel a WGRAD_KERNELS name, None where the fc is a plain
    GEMM), "tail" (CPW, item-gradient kernel, IT, WLDS, items of the last workgroup)."""
    buf = (ctypes.c_int32 * LAUNCH_SHAPE_WORDS)()
    check(lib().dcue_debug_launch_shape(ctypes.byref(dims), layout, B, N, M, ctypes.cast(buf, _P),
                                        LAUNCH_SHAPE_WORDS), "dcue_debug_launch_shape")
    w = list(buf)
    wg = {}
    for l in range(1, 7):
        k, nch, rpc, last = w[45 + 4 * (l - 1):45 + 4 * l]
        wg[l] = (WGRAD_KERNELS[k] if k >= 0 else None, nch, rpc, last)
    return {"fwd": {l: tuple(w[5 * (l - 1):5 * l]) for l in range(1, 6)},
            "dgrad": {l: tuple(w[25 + 5 * (l - 2):25 + 5 * (l - 1)]) for l in range(2, 6)},
            "wgrad": wg, "tail": tuple(w[69:74])}


TEXT_SHAPE_WORDS = 16  # DCUE_TEXT_SHAPE_WORDS
_TEXT_FWD_FIELDS = ("kernel", "tb", "waves", "nct", "bpd", "nch", "nxcd", "units", "grid", "lds", "lds_static", "last")
_TEXT_WGRAD_FIELDS = ("nchunk", "items_per_chunk", "last", "reduce")


def text_shape(dims, M):
    """The text branch's launches over M items (dcue_debug_text_shape; host only, no GPU needed):
    {"fwd": {kernel "full" / "chunked", tb (TBW / TB), waves (chunked: items per workgroup), nct, bpd,
    nch, nxcd, units, grid, lds, lds_static, last (items of the last workgroup)}, "wgrad": {nchunk,
    items_per_chunk, last (items of the last chunk), reduce}}."""
    buf = (ctypes.c_int32 * TEXT_SHAPE_WORDS)()
    check(lib().dcue_debug_text_shape(ctypes.byref(dims), M, ctypes.cast(buf, _P), TEXT_SHAPE_WORDS),
          "dcue_debug_text_shape")
    w = list(buf)
    fwd = dict(zip(_TEXT_FWD_FIELDS, w[:12]))
    fwd["kernel"] = "chunked" if fwd["kernel"] else "full"
    wg = dict(zip(_TEXT_WGRAD_FIELDS, w[12:16]))
    wg["reduce"] = bool(wg["reduce"])
    return {"fwd": fwd, "wgrad": wg}


def workspace_text(dims, B, N, M):
    """Byte offsets of the text branch's (xfc [M][text_dim + d_s] float, dtp [M][C_s] float, tidx
    [M][C_s] uint8) inside a (B, N, M) workspace; an error outside the text tower."""
    off = (ctypes.c_size_t * 3)()
    check(lib().dcue_workspace_text(ctypes.byref(dims), B, N, M, off), "dcue_workspace_text")
    return list(off)


def debug_delay(site, microseconds):
    """Spin `microseconds` on the stream of the step's work at `site` (a DEBUG_SITES name or index)
    before that work, in every later step (include/dcue.h dcue_debug_delay); 0 turns it off."""
    i = DEBUG_SITES.index(site) if isinstance(site, str) else int(site)
    check(lib().dcue_debug_delay(i, int(microseconds)), "dcue_debug_delay")


def debug_clear_delays():
    for i in range(len(DEBUG_SITES)):
        check(lib().dcue_debug_delay(i, 0), "dcue_debug_delay")


def debug_fail_flags():
    """Read and clear the fused user-tower forward's gave-up flag (dcue_debug_fail_flags)."""
    v = ctypes.c_uint32()
    check(lib().dcue_debug_fail_flags(ctypes.byref(v)), "dcue_debug_fail_flags")
    return v.value


def crop_config(mode, seed=0, draw=0, grid_j=0, grid_n=1):
    """dcue_crop_config for a DCUE_CROP_* mode (include/dcue.h has the window rule)."""
    return CropConfig(int(mode), int(grid_j), int(grid_n), 0, int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1))


def track_store(data, frame_ptr):
    """dcue_track_store over data [total_frames][128] (fp16 / fp32) and frame_ptr int64 [n_tracks + 1],
    both device tensors."""
    if data.dtype not in (torch.float16, torch.float32) or frame_ptr.dtype != torch.int64:
        raise ValueError("track store: data must be fp16 or fp32 and frame_ptr int64")
    if data.dim() != 2 or data.shape[1] != N_MELS or not data.is_contiguous() or frame_ptr.numel() < 1:
        raise ValueError("track store: data must be a contiguous [total_frames][%d]" % N_MELS)
    return TrackStore(data.data_ptr(), frame_ptr.data_ptr(), frame_ptr.numel() - 1, data.shape[0],
                      0 if data.dtype == torch.float16 else 1, 0)


def augment_config(freq_masks=0, freq_width=0, time_masks=0, time_width=0, gain_db=0.0, fill="mean"):
    """dcue_augment_config (include/dcue.h has the rule): fill is 'mean' or the constant a masked
    element becomes. The library checks the ranges."""
    mean = isinstance(fill, str)
    if mean and fill != "mean":
        raise ValueError("augment: fill must be 'mean' or a number, got %r" % (fill,))
    return AugmentConfig(int(freq_masks), int(freq_width), int(time_masks), int(time_width), float(gain_db),
                         AUG_FILL_MEAN if mean else AUG_FILL_CONST, 0.0 if mean else float(fill), 0)


def crop_tracks(data, frame_ptr, cfg, out, rows=None, starts=None, flags=None, stream=None, augment=None):
    """dcue_crop_tracks: out [n_out][131][128] (fp16 / fp32) receives the window of track rows[i] (int32;
    None: track i) of the store (data, frame_ptr). Returns the flags tensor (int32 [n_out], device).
    augment (an augment_config): dcue_crop_tracks_augmented, the same windows masked and gain-shifted."""
    n_out = int(out.shape[0])
    if out.dim() != 3 or tuple(out.shape[1:]) != (N_FRAMES, N_MELS) or not out.is_contiguous():
        raise ValueError("crop_tracks: out must be a contiguous [n][%d][%d]" % (N_FRAMES, N_MELS))
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != n_out):
        raise ValueError("crop_tracks: rows must be int32 [n_out]")
    if flags is None:
        flags = torch.empty(max(n_out, 1), dtype=torch.int32, device=out.device)
    store = track_store(data, frame_ptr)
    tail = (n_out, ptr(out), 0 if out.dtype == torch.float16 else 1, ptr(starts), ptr(flags),
            stream_handle(out.device) if stream is None else stream)
    if augment is None:
        check(lib().dcue_crop_tracks(ctypes.byref(store), ctypes.byref(cfg), ptr(rows), *tail), "dcue_crop_tracks")
    else:
        check(lib().dcue_crop_tracks_augmented(ctypes.byref(store), ctypes.byref(cfg), ctypes.byref(augment), ptr(rows),
                                               *tail), "dcue_crop_tracks_augmented")
    return flags[:n_out]


def select_negatives(user_feat, item_feat, users, pool, N, H, out=None, out_hard=None, out_flags=None, stream=None):
    """dcue_select_negatives: out of pool [n, P] (int64 item indices) keep per row the H that the fp32
    factors user_feat [n_users, d] / item_feat [n_items, d] score highest for users [n], filled up to N
    with the pool's other draws in order. Returns (out [n, N] int64, out_hard [n] int32, out_flags [n]
    int32), device tensors; the call does not wait for its stream."""
    for name, x, dt in (("user_feat", user_feat, torch.float32), ("item_feat", item_feat, torch.float32),
                        ("users", users, torch.int64), ("pool", pool, torch.int64)):
        require_gpu(x, name)
        if x.dtype != dt or not x.is_contiguous():
            raise ValueError("select_negatives: %s must be a contiguous %s tensor" % (name, dt))
    if user_feat.dim() != 2 or item_feat.dim() != 2 or user_feat.shape[1] != item_feat.shape[1]:
        raise ValueError("select_negatives: user_feat and item_feat must be [rows, d] with one d")
    n = users.numel()
    if pool.dim() != 2 or pool.shape[0] != n:
        raise ValueError("select_negatives: pool must be [len(users), P]")
    dev = pool.device
    out = torch.empty((n, max(int(N), 0)), dtype=torch.int64, device=dev) if out is None else out
    out_hard = torch.empty(n, dtype=torch.int32, device=dev) if out_hard is None else out_hard
    out_flags = torch.empty(n, dtype=torch.int32, device=dev) if out_flags is None else out_flags
    for name, x, dt, numel in (("out", out, torch.int64, n * int(N)), ("out_hard", out_hard, torch.int32, n),
                               ("out_flags", out_flags, torch.int32, n)):
        if x.dtype != dt or not x.is_contiguous() or x.numel() != numel:
            raise ValueError("select_negatives: %s must be a contiguous %s tensor of %d elements" % (name, dt, numel))
    if n == 0:  # empty tensors have no address to pass
        return out, out_hard, out_flags
    check(lib().dcue_select_negatives(ptr(user_feat), user_feat.shape[0], ptr(item_feat), item_feat.shape[0],
                                      user_feat.shape[1], ptr(users), ptr(pool), n, pool.shape[1], int(N), int(H),
                                      ptr(out), ptr(out_hard), ptr(out_flags),
                                      stream_handle(dev) if stream is None else stream), "dcue_select_negatives")
    return out, out_hard, out_flags


def crop_starts_host(cfg, lengths, track_ids=None):
    """dcue_crop_starts_host: the window's first frame for tracks of `lengths` frames at store indices
    `track_ids` (default 0..n-1), as an int64 numpy array. No GPU needed."""
    import numpy as np
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    ids = None if track_ids is None else np.ascontiguousarray(track_ids, dtype=np.int64)
    out = np.zeros(len(lengths), dtype=np.int64)
    check(lib().dcue_crop_starts_host(ctypes.byref(cfg), ctypes.c_void_p(lengths.ctypes.data),
                                      None if ids is None else ctypes.c_void_p(ids.ctypes.data), len(lengths),
                                      ctypes.c_void_p(out.ctypes.data)), "dcue_crop_starts_host")
    return out


def augment_params_host(cfg, augment, lengths, track_ids=None):
    """dcue_augment_params_host: what the augmentation rule gives tracks of `lengths` frames at store
    indices `track_ids` (default 0..n-1): (gain float32 [n], freq_pw int32 [n][4][2], time_pw int32
    [n][4][2]), the masks as (place, width). No GPU needed."""
    import numpy as np
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    ids = None if track_ids is None else np.ascontiguousarray(track_ids, dtype=np.int64)
    n = len(lengths)
    gain = np.zeros(n, dtype=np.float32)
    freq_pw = np.zeros((n, AUG_MAX_MASKS, 2), dtype=np.int32)
    time_pw = np.zeros((n, AUG_MAX_MASKS, 2), dtype=np.int32)
    check(lib().dcue_augment_params_host(ctypes.byref(cfg), ctypes.byref(augment), ctypes.c_void_p(lengths.ctypes.data),
                                         None if ids is None else ctypes.c_void_p(ids.ctypes.data), n,
                                         ctypes.c_void_p(gain.ctypes.data), ctypes.c_void_p(freq_pw.ctypes.data),
                                         ctypes.c_void_p(time_pw.ctypes.data)), "dcue_augment_params_host")
    return gain, freq_pw, time_pw
