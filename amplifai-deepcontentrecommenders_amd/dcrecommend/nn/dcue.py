"""DCUE trainer on MI355X: the reference's dcrecommend.nn.dcue.DCUE (nn/dcue.py:43-785).

Same constructor arguments and attributes, the same fit / score / score_song / predict /
predict_song / save / load / insert_best_factors / get_item_factors methods and the same
sub-epoch loop (10 shuffled chunks per epoch, a val pass, factors and AUC/mAP after each chunk,
best-by-val-mAP checkpoints), so a train script written against the reference runs unchanged.

What runs where:
* spectrograms are loaded ONCE into an HBM table (DCUEItemset.track_table) instead of 21
  torch.loads per row in DataLoader workers;
* per batch: catalogue negatives on the GPU (MT19937 continuing numpy's global stream, the
  reference's num_workers=0 draw order), then one TrainPlan step (forward, hinge, backward,
  NativeAdam, include/dcue.h dcue_plan_step) and the cyclic LR schedule;
* item / user factors through the eval towers (dcue_item_tower_eval, dcue_user_tower);
* AUC / mAP through dcue_rank_metrics (dcrecommend.nn.rank) instead of per-user pandas frames
  and sklearn calls.
The only host work per batch is the index permutation (torch RandomSampler, as the reference's
DataLoader(shuffle=True)) and the kernel launches. numpy's and torch's global random streams are
consumed as the reference consumes them with num_workers=0 loaders (negative draws continue numpy's
stream on the GPU; every DataLoader iteration's torch draws are mirrored), so a seeded fit follows
the reference's trajectory: tests/golden/fit.npz.
"""
import ctypes
import dataclasses
import math
import os
import warnings

import numpy as np
import torch
from torch.utils.data import RandomSampler

from dcrecommend import _native as nat
from dcrecommend.datasets import popularity as _pop
from dcrecommend.datasets.artists import artist_exclusion_csr, artist_groups
from dcrecommend.datasets.csr import (check_catalogue_users, saturated_users, user_split_ranks,
                                      weighted_saturated_users, weighted_split_tables)
from dcrecommend.dcue.dcue import DCUENet
from dcrecommend.dcue.plan import TrainPlan
from dcrecommend.nn import rank
from dcrecommend.nn.trainer import Trainer
from dcrecommend.optim import NativeAdam, NativeRanger, NativeSGD
from dcrecommend.optim.cyclic_scheduler import CyclicLRWithRestarts


def _dataset(x):
    """The reference passes DataLoaders around; accept a loader or its dataset."""
    return getattr(x, "dataset", x)


def _loader_draws(n):
    """The draws n DataLoader iterations take from torch's global RNG: each iterator draws a base
    seed (torch/utils/data/dataloader.py _BaseDataLoaderIter), so torch's stream -- and with it every
    later RandomSampler permutation -- stays where the reference's trainer leaves it."""
    for _ in range(n):
        torch.empty((), dtype=torch.int64).random_()


class _IndexBatches:
    """One sub-epoch loader (nn/dcue.py:711-721): the rows of a get_batches chunk in
    RandomSampler order (DataLoader(shuffle=True)), cut into batches, drop_last. Iterating takes the
    same two draws from torch's global RNG as the DataLoader: its base seed, then the sampler's."""

    def __init__(self, rows, batch_size):
        self.rows = np.asarray(rows, dtype=np.int64)
        self.batch_size = batch_size

    def __len__(self):
        return len(self.rows) // self.batch_size

    def __iter__(self):
        _loader_draws(1)
        order = np.fromiter(iter(RandomSampler(range(len(self.rows)))), dtype=np.int64, count=len(self.rows))
        rows = self.rows[order]
        B = self.batch_size
        for b in range(len(self)):
            yield rows[b * B:(b + 1) * B]


class _Negatives:
    """GPU catalogue sampler over one split (datasets/dcuedataset.py:207-220): the user -> split-rank
    CSR, the split's item list and the MT19937 stream on the device. A dataset whose neg_sampling is
    not 'uniform' draws in proportion to its negative_weights() (dcue_sample_catalogue_weighted)."""

    def __init__(self, ds, device):
        self.ds = ds
        self.device = device
        split = ds.split_items()
        coo = ds.item_user.tocoo()
        indptr, ranks = user_split_ranks(coo.col, coo.row, ds.n_users, split)
        self.split = torch.from_numpy(split).to(device)
        self.indptr = torch.from_numpy(indptr).to(device)
        self.ranks = torch.from_numpy(ranks if len(ranks) else np.zeros(1, np.int32)).to(device)
        self.reseed = ds.random_seed is not None
        self.seed = int(ds.random_seed) if self.reseed else 0
        self.saturated = saturated_users(indptr, len(split))  # usually empty
        self.tables = None
        if getattr(ds, "neg_sampling", "uniform") != "uniform":
            host = weighted_split_tables(indptr, ranks, ds.negative_weights())
            self.saturated = weighted_saturated_users(host[3])
            # the struct holds addresses: the tensors stay referenced beside it
            self._tables = [torch.from_numpy(a if len(a) else np.zeros(1, np.uint32)).to(device) for a in host]
            self.tables = nat.WeightTables(*[t.data_ptr() for t in self._tables])

    def check(self, users):
        """ValueError (numpy's) before a batch whose user has no candidate negative is sampled."""
        if len(self.saturated):
            check_catalogue_users(users.cpu().numpy() if torch.is_tensor(users) else users, self.saturated)

    def draw(self, mt, users, N, out, stream=None):
        if self.tables is not None:
            nat.check(nat.lib().dcue_sample_catalogue_weighted(
                None if self.reseed else nat.ptr(mt), int(self.reseed), self.seed, nat.ptr(self.split),
                self.split.numel(), nat.ptr(self.indptr), nat.ptr(self.ranks), ctypes.byref(self.tables),
                nat.ptr(users), users.numel(), N, nat.ptr(out),
                nat.stream_handle(self.device) if stream is None else stream), "dcue_sample_catalogue_weighted")
            return
        nat.check(nat.lib().dcue_sample_catalogue(
            None if self.reseed else nat.ptr(mt), int(self.reseed), self.seed, nat.ptr(self.split),
            self.split.numel(), nat.ptr(self.indptr), nat.ptr(self.ranks), nat.ptr(users), users.numel(), N,
            nat.ptr(out), nat.stream_handle(self.device) if stream is None else stream), "dcue_sample_catalogue")


def _mt_from_numpy(device):
    """numpy's global MT19937 state as a device dcue_mt_state (624 words + position)."""
    name, key, pos = np.random.get_state()[:3]
    buf = np.zeros(nat.MT_STATE_BYTES // 4, dtype=np.uint32)
    buf[:624] = key
    buf[624] = np.uint32(pos)
    return torch.from_numpy(buf.view(np.uint8).copy()).to(device)


def _mt_to_numpy(mt):
    """Continue numpy's global stream where the device stream stopped."""
    buf = mt.cpu().numpy().view(np.uint32)
    np.random.set_state(("MT19937", buf[:624].copy(), int(buf[624]), 0, 0.0))


@dataclasses.dataclass
class Augment:
    """DCUE(augment=...): SpecAugment-style masks and a loudness jitter applied while the training table
    is re-cut (include/dcue.h dcue_crop_tracks_augmented has the rule). Up to 4 frequency masks of at
    most freq_width mel bins and 4 time masks of at most time_width frames per track, a gain drawn from
    [-gain_db, gain_db) per track; fill: what a masked element becomes, 'mean' (the window's mean) or a
    number."""
    freq_masks: int = 0
    freq_width: int = 0
    time_masks: int = 0
    time_width: int = 0
    gain_db: float = 0.0
    fill: object = 'mean'


class DCUE(Trainer):

    def __init__(self, feature_dim=100, conv_hidden=128, batch_size=64, neg_batch_size=20, u_embdim=300,
                 margin=0.2, optimize='adam', lr=0.00001, beta_one=0.9, beta_two=0.99, eps=1e-8,
                 weight_decay=0, restart_period=30, t_mult=2, num_epochs=90, model_type='truedcuemel1dbn',
                 eval_pct=0.025, val_pct=1.0, device=None, defer_embedding=True, crop='load', crop_seed=0,
                 factor_crops='random', neg_pool=None, neg_hard=None, augment=None):
        """Arguments as nn/dcue.py:47-50; device (default cuda:current) and defer_embedding (the
        bit-identical deferred user-table Adam, dcrecommend.optim.NativeAdam) are MI355X additions.

        crop: 'load' cuts each track's 131-frame window once, when the catalogue is loaded. 'epoch'
        keeps the full-length tracks in HBM (DCUEItemset.track_store) and re-cuts the whole table in
        place before every training sub-epoch, a random window per track from (crop_seed, nn_epoch)
        (include/dcue.h dcue_crop_tracks); the item factors then average n_iter real passes over
        factor_crops windows: 'random' (the same draws every epoch) or 'grid' (evenly spread).

        neg_pool=P (N <= P <= 1024, N the negatives per row) turns hard negatives on for the training
        sub-epochs: every row draws P candidates where it drew N, and keeps the neg_hard (default N // 2;
        0 <= neg_hard <= N) that the factors of the last sub-epoch score highest for its user, filled up
        to N with the pool's leading other draws (include/dcue.h dcue_select_negatives). None, the
        default, is the plain sampler. Validation and test losses always use N plain draws.

        augment (an Augment or a dict of its fields; crop='epoch' only) masks and gain-shifts the windows
        of the training sub-epochs' re-crop, from (crop_seed, nn_epoch) like the windows themselves.
        Validation losses, the item factors and embed_audio always see the clean windows. None, the
        default, is the plain re-crop."""
        self._check_neg_pool(neg_pool, neg_hard)
        augment = self._check_augment(augment, crop)
        if crop not in ('load', 'epoch'):
            raise ValueError("crop must be 'load' or 'epoch', got %r" % (crop,))
        if factor_crops not in ('random', 'grid'):
            raise ValueError("factor_crops must be 'random' or 'grid', got %r" % (factor_crops,))
        Trainer.__init__(self)
        self.crop = crop
        self.crop_seed = int(crop_seed)
        self.factor_crops = factor_crops
        self.augment = augment    # None, or the Augment's fields as a plain dict (a checkpoint keeps it)
        self._tracks_dirty = False  # the table holds augmented windows, cut at draw _tracks_draw
        self._tracks_draw = 0
        self.neg_pool = None if neg_pool is None else int(neg_pool)
        self.neg_hard = None if neg_hard is None else int(neg_hard)
        self._on_negatives = None  # tests: called as (step, users, pool, negs, hard) on the sampling stream
        self.feature_dim = feature_dim
        self.conv_hidden = conv_hidden
        self.batch_size = batch_size
        self.neg_batch_size = neg_batch_size
        self.u_embdim = u_embdim
        self.margin = margin
        self.optimize = optimize
        self.lr = lr
        self.beta_one = beta_one
        self.beta_two = beta_two
        self.eps = eps
        self.weight_decay = weight_decay
        self.restart_period = restart_period
        self.t_mult = t_mult
        self.num_epochs = num_epochs
        self.model_type = model_type
        self.eval_pct = eval_pct
        self.val_pct = val_pct
        self.n_users = None
        self.n_items = None
        self.epoch_size = None
        self.model_dir = None
        self.train_data = self.val_data = self.test_data = None
        self.pred_data = self.truth_data = self.item_data = None
        self.model = None
        self.optimizer = None
        self.scheduler = None
        self.loss_func = None
        self.dict_args = None
        self.nn_epoch = 0
        self.item_factors = None
        self.user_factors = None
        self.best_item_factors = None
        self.best_user_factors = None
        self.best_val_map = 0
        self.best_val_auc = 0
        self.best_val_loss = float('inf')
        self.metadata_path = None
        self.triplets_path = None
        self.USE_CUDA = True
        self.device = torch.device(device if device is not None else "cuda")
        self.defer_embedding = defer_embedding
        self._tracks = None       # [n_items][131][128] HBM table, item-index order
        self._store = None        # crop='epoch': (data [total_frames][128], frame_ptr [n_items + 1]) beside it
        self._item_meta = None    # metadata index of every item index
        self._plan = None
        self._plan_n = None
        self._evals = {}
        self._song_artist_map = None  # set_artists
        self._popularity = None  # set_popularity: the {song_id: count} dict, or "train"

    # ------------------------------------------------------------------ model / optimizer
    def _init_nn(self, audio_model=None):
        self.dict_args = {'feature_dim': self.feature_dim, 'conv_hidden': self.conv_hidden,
                          'user_embdim': self.u_embdim, 'user_count': self.n_users,
                          'model_type': self.model_type}
        self.model = DCUENet(self.dict_args)
        if audio_model is not None:
            sd = self.model.state_dict()
            sd.update(audio_model)
            self.model.load_state_dict(sd)
        self.model = self.model.to(self.device)
        if self.optimize == 'adam':
            self.optimizer = NativeAdam(self.model.parameters(), self.lr, (self.beta_one, self.beta_two), self.eps,
                                        self.weight_decay, defer_embedding=self.defer_embedding)
        elif self.optimize == 'sgd':
            # nn/dcue.py:148-152; its StepLR(optimizer, 1, 1 - 1e-6) is replaced by the cyclic schedule
            # right after (:159) and never stepped, so it changes nothing
            self.optimizer = NativeSGD(self.model.parameters(), self.lr, self.beta_one,
                                       weight_decay=self.weight_decay, nesterov=True)
        elif self.optimize == 'ranger':
            self.optimizer = NativeRanger(self.model.parameters(), lr=self.lr, alpha=0.5, k=6, N_sma_threshhold=5,
                                          betas=(self.beta_one, self.beta_two), eps=1e-5,
                                          weight_decay=self.weight_decay)
        else:
            # the reference leaves self.optimizer None and its scheduler raises TypeError
            # (nn/dcue.py:159-162, optim/cyclic_scheduler.py)
            self.optimizer = None
        self.scheduler = CyclicLRWithRestarts(self.optimizer, self.batch_size, epoch_size=self.epoch_size,
                                              restart_period=self.restart_period, t_mult=self.t_mult,
                                              policy='cosine')
        self._plan = None

    def _loss_func(self, preds):
        """nn/dcue.py:167-170."""
        return torch.max(torch.zeros_like(preds), self.margin - preds).sum(dim=1).mean()

    # ------------------------------------------------------------------ device data
    def _bind_items(self, item_dataset):
        """Load the catalogue once: track table in item-index order, item -> metadata row map."""
        if self._tracks is not None and self._tracks_src is item_dataset:
            return
        meta = item_dataset.item_rows()
        if self.crop == 'epoch':
            data, frame_ptr = item_dataset.track_store(self.device)
            self._store = (data, frame_ptr)
            self._tracks = torch.empty((len(meta), nat.N_FRAMES, nat.N_MELS), dtype=data.dtype, device=self.device)
            self._plan = None  # a plan binds the table's address
            bad = int(self._recrop().count_nonzero())
            if bad:
                raise RuntimeError("track store: %d tracks with an extent outside the store" % bad)
        else:
            table_meta = item_dataset.track_table(self.device, n_meta=max(len(item_dataset.songid2metaindex), 1))
            rows = torch.from_numpy(np.where(meta >= 0, meta, 0)).to(self.device)
            self._tracks = table_meta.index_select(0, rows).contiguous()
            self._store = None
        self._item_meta = meta
        self._tracks_src = item_dataset

    def _recrop(self, draw=None, augment=False):
        """crop='epoch': cut the whole track table again, in place, into the buffer the plan is bound
        to -- a random window of every track from (crop_seed, draw), draw = nn_epoch by default, the
        same on every rank. Returns the call's flags (device). Only at an epoch boundary: the plan must
        hold no lookahead (it would feed the next step statistics of the old rows), and this stream
        first waits for what the last step left on the plan's side streams, which read the table.

        augment=True (the training sub-epoch's re-crop alone) applies self.augment in the same launch
        and leaves the table marked dirty: _clean_tracks cuts the same windows again, clean."""
        data, frame_ptr = self._store
        if self._plan is not None:
            self._plan.require_no_lookahead()
            self._plan.sync(nat.stream_handle(self.device))
        draw = self.nn_epoch if draw is None else draw
        cfg = nat.crop_config(nat.CROP_RANDOM, seed=self.crop_seed, draw=draw)
        if not augment or self.augment is None:  # exactly the call there was before there was an augment
            flags = nat.crop_tracks(data, frame_ptr, cfg, self._tracks)
            self._tracks_dirty = False
        else:
            flags = nat.crop_tracks(data, frame_ptr, cfg, self._tracks, augment=nat.augment_config(**self.augment))
            a = self.augment  # an augment that is off runs the plain kernel: nothing to undo
            self._tracks_dirty = bool(a["freq_masks"] * a["freq_width"] or a["time_masks"] * a["time_width"]
                                      or a["gain_db"])
        self._tracks_draw = draw
        return flags

    def _clean_tracks(self):
        """Before anything outside the training sub-epoch reads the table: if it holds augmented windows,
        cut the same windows -- the same (crop_seed, draw) -- again without the augmentation. A table
        that is clean already is left alone, so an evaluation after an evaluation re-cuts nothing."""
        if self._store is not None and self._tracks_dirty:
            self._recrop(draw=self._tracks_draw)

    @staticmethod
    def _check_augment(augment, crop):
        """ValueError for an augment no re-crop could run with. Returns the fields as a plain dict, or
        None with the augmentation off."""
        if augment is None:
            return None
        if isinstance(augment, Augment):
            augment = dataclasses.asdict(augment)
        elif not isinstance(augment, dict):
            raise ValueError("augment must be an Augment or a dict of its fields, got %r" % (augment,))
        names = [f.name for f in dataclasses.fields(Augment)]
        unknown = sorted(set(augment) - set(names))
        if unknown:
            raise ValueError("augment: unknown fields %s (known: %s)" % (", ".join(unknown), ", ".join(names)))
        a = dataclasses.asdict(Augment(**augment))
        for name, top in (("freq_masks", nat.AUG_MAX_MASKS), ("freq_width", nat.N_MELS),
                          ("time_masks", nat.AUG_MAX_MASKS), ("time_width", nat.N_FRAMES)):
            v = a[name]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= top:
                raise ValueError("augment: %s must be an integer in 0..%d, got %r" % (name, top, v))
            a[name] = int(v)
        try:
            a["gain_db"] = float(a["gain_db"])
        except (TypeError, ValueError):
            raise ValueError("augment: gain_db must be a number, got %r" % (a["gain_db"],))
        if not (math.isfinite(a["gain_db"]) and a["gain_db"] >= 0):
            raise ValueError("augment: gain_db must be finite and >= 0, got %r" % (a["gain_db"],))
        if a["fill"] != 'mean':
            if isinstance(a["fill"], (str, bool)) or not isinstance(a["fill"], (int, float, np.number)) \
                    or not math.isfinite(a["fill"]):
                raise ValueError("augment: fill must be 'mean' or a finite number, got %r" % (a["fill"],))
            a["fill"] = float(a["fill"])
        if crop != 'epoch':
            raise ValueError("augment needs crop='epoch': with crop=%r there is no store to re-cut" % (crop,))
        return a

    @staticmethod
    def _check_neg_pool(neg_pool, neg_hard, N=None):
        """ValueError for a neg_pool / neg_hard pair no sub-epoch could run with; the bounds against N
        once it is known. Returns (P, H), or None with the mode off."""
        if neg_pool is None:
            if neg_hard is not None:
                raise ValueError("neg_hard needs neg_pool: without a pool there is nothing to select from")
            return None
        for name, v in (("neg_pool", neg_pool), ("neg_hard", neg_hard)):
            if v is not None and (isinstance(v, bool) or int(v) != v):
                raise ValueError("%s must be an integer, got %r" % (name, v))
        P = int(neg_pool)
        if not 1 <= P <= nat.SELECT_MAX_POOL:
            raise ValueError("neg_pool must be in 1..%d, got %d" % (nat.SELECT_MAX_POOL, P))
        if neg_hard is not None and not 0 <= int(neg_hard) <= P:
            raise ValueError("neg_hard must be in 0..neg_pool, got %d" % int(neg_hard))
        if N is None:
            return P, neg_hard
        if P < N:
            raise ValueError("neg_pool must be at least the %d negatives per row, got %d" % (N, P))
        H = N // 2 if neg_hard is None else int(neg_hard)
        if H > N:
            raise ValueError("neg_hard must be at most the %d negatives per row, got %d" % (N, H))
        return P, H

    def _n_neg(self, ds):
        """Negatives per row: the dataset's neg_samples, as in the reference, where the trainer's
        neg_batch_size is never read (datasets/dcuedataset.py:18,219)."""
        return int(getattr(ds, "neg_samples", self.neg_batch_size))

    def _train_plan(self, N):
        if self._plan is None or self._plan_n != N:
            self._plan = TrainPlan(self.model, self._tracks, self.batch_size, N,
                                   margin=self.margin, optimizer=self.optimizer)
            self._plan_n = N
        return self._plan

    # ------------------------------------------------------------------ epochs
    def _train_epoch(self, loader):
        """nn/dcue.py:172-218: per batch sample negatives, forward, hinge, backward, Adam, LR step.

        The reference draws each row's catalogue negatives in its DataLoader workers, ahead of the
        step that consumes them (datasets/dcuedataset.py:207-256). Here the batches' negatives are
        drawn two steps ahead on a sampling stream -- in batch order on the one numpy-compatible
        MT19937 stream, so the very same negatives -- and each batch's item list is built there too,
        so the plan also prepares the next batch's bn0 statistics beside the current step.

        With neg_pool=P each row draws P candidates there instead -- still the one stream, P draws per
        row -- and dcue_select_negatives keeps the neg_hard that the factors score highest for the
        row's user, on the sampling stream too, so the step schedule is the same. The factors are a
        snapshot from the start of the sub-epoch: fit leaves them one sub-epoch old."""
        ds = loader.dataset if hasattr(loader, "dataset") else self.train_data
        neg = self._negatives(ds)
        B, N = self.batch_size, self._n_neg(ds)
        select = self._check_neg_pool(self.neg_pool, self.neg_hard, N)
        if select is not None:
            if self.user_factors is None or self.item_factors is None:
                # called outside fit: once, and torch's global stream (the batch order) stays put
                item_data = self.item_data if self.item_data is not None else self._tracks_src
                with torch.random.fork_rng(devices=[]):
                    self._user_factors(item_data)
                    self._item_factors(item_data)
            P, H = select
            user_feat = self.user_factors.contiguous()
            item_feat = self._item_feat_by_index().contiguous()
        self.model.train()
        plan = self._train_plan(N)
        if self._store is not None:
            # before the sampling stream joins the main one below: every later reader of the table --
            # the steps and the lookaheads they start -- is ordered after this stream's re-crop
            self._recrop(augment=True)
        users_all, items_all = self._rows(ds)
        batches = list(loader)  # the loader's RNG draws happen when its iteration starts, as before
        dev = self.device
        main = torch.cuda.current_stream(dev)
        samp = torch.cuda.Stream(device=dev)
        mt = _mt_from_numpy(dev)
        users = [torch.empty(B, dtype=torch.int64, device=dev) for _ in range(3)]
        pos = [torch.empty(B, dtype=torch.int64, device=dev) for _ in range(3)]
        negs = [torch.empty((B, N), dtype=torch.int64, device=dev) for _ in range(3)]
        items = [torch.empty(B * (1 + N), dtype=torch.int32, device=dev) for _ in range(3)]
        ready = [torch.cuda.Event() for _ in range(3)]
        done = [torch.cuda.Event() for _ in range(3)]
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        if select is not None:
            pool = [torch.empty((B, P), dtype=torch.int64, device=dev) for _ in range(3)]
            hard = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3)]
            # every batch's flags stay on the device to the end of the sub-epoch: nothing waits for them
            flags = torch.zeros((max(len(batches), 1), B), dtype=torch.int32, device=dev)
            select_fn = nat.lib().dcue_select_negatives
            feat_args = (nat.ptr(user_feat), user_feat.shape[0], nat.ptr(item_feat), item_feat.shape[0],
                         user_feat.shape[1])
        samp.wait_stream(main)  # the sampler state, the row tables and the factors: written on the main stream

        def prepare(s):
            k = s % 3
            with torch.cuda.stream(samp):
                r = torch.from_numpy(batches[s]).to(dev)
                torch.index_select(users_all, 0, r, out=users[k])
                torch.index_select(items_all, 0, r, out=pos[k])
                neg.check(users[k])
                if select is None:
                    neg.draw(mt, users[k], N, negs[k], stream=samp.cuda_stream)
                else:
                    neg.draw(mt, users[k], P, pool[k], stream=samp.cuda_stream)
                    nat.check(select_fn(*feat_args, nat.ptr(users[k]), nat.ptr(pool[k]), B, P, N, H, nat.ptr(negs[k]),
                                        nat.ptr(hard[k]), ctypes.c_void_p(flags.data_ptr() + 4 * B * s),
                                        samp.cuda_stream), "dcue_select_negatives")
                    if self._on_negatives is not None:
                        self._on_negatives(s, users[k], pool[k], negs[k], hard[k])
                nat.check(nat.lib().dcue_build_catalogue_batch(nat.ptr(pos[k]), nat.ptr(negs[k]), B, N,
                                                               nat.ptr(items[k]), samp.cuda_stream),
                          "dcue_build_catalogue_batch")
                ready[k].record(samp)

        n = len(batches)
        for s in range(min(2, n)):
            prepare(s)
        for s in range(n):
            main.wait_event(ready[min(s + 1, n - 1) % 3])  # this batch and the next one are built
            if s + 1 < n:
                plan.set_next(items[(s + 1) % 3])
            plan.step(users[s % 3], items[s % 3])
            self.scheduler.batch_step()
            loss_sum += plan.loss.double() * B
            done[s % 3].record(main)
            if s + 2 < n:  # buffers (s+2) % 3 were batch s-1's
                if s >= 1:
                    samp.wait_event(done[(s - 1) % 3])
                prepare(s + 2)
        main.wait_stream(samp)
        _mt_to_numpy(mt)
        if select is not None:
            # one device word, read once: nothing waited for the flags while the steps ran
            word = int((flags & nat.SELECT_FLAG_NONFINITE).max() | (flags & nat.SELECT_FLAG_BAD_ID).max())
            if word & nat.SELECT_FLAG_BAD_ID:
                raise RuntimeError("hard negatives: a user or item index lies outside the factor tables "
                                   "(%d users, %d items): the factors do not belong to this dataset"
                                   % (user_feat.shape[0], item_feat.shape[0]))
            if word & nat.SELECT_FLAG_NONFINITE:
                warnings.warn("hard negatives: a factor score was NaN or infinite during this sub-epoch; "
                              "a NaN score is never chosen as hard", RuntimeWarning)
        return n * B, float(loss_sum) / max(n * B, 1)

    def _eval_epoch(self, loader):
        """nn/dcue.py:220-262: eval-mode loss over the val set in order (last batch partial)."""
        _loader_draws(1)  # DataLoader(shuffle=False): its iterator's base seed
        self._clean_tracks()  # the validation loss is computed on the windows as recorded
        self.model.eval()
        ds = _dataset(loader)
        neg = self._negatives(ds)
        users_all, items_all = self._rows(ds)
        B, N = self.batch_size, self._n_neg(ds)
        mt = _mt_from_numpy(self.device)
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        n = users_all.numel()
        for s in range(0, n, B):
            users = users_all[s:s + B].contiguous()
            b = users.numel()
            negs = torch.empty((b, N), dtype=torch.int64, device=self.device)
            neg.check(users)
            neg.draw(mt, users, N, negs)
            track = torch.empty(b * (1 + N), dtype=torch.int32, device=self.device)
            nat.check(nat.lib().dcue_build_catalogue_batch(nat.ptr(items_all[s:s + B].contiguous()), nat.ptr(negs),
                                                           b, N, nat.ptr(track), nat.stream_handle()),
                      "dcue_build_catalogue_batch")
            _, _, _, loss = self.model.native_forward(users, self._tracks, track, N, nat.LAYOUT_CATALOGUE,
                                                      train=False, margin=self.margin, copy_outputs=False)
            loss_sum += loss.double() * b
        _mt_to_numpy(mt)
        return n, float(loss_sum) / max(n, 1)

    def _negatives(self, ds):
        key = ("neg", id(ds))
        if key not in self._evals:
            self._evals[key] = _Negatives(ds, self.device)
        return self._evals[key]

    def _rows(self, ds):
        key = ("rows", id(ds), len(ds))
        if key not in self._evals:
            u, s = ds.split_rows()
            self._evals[key] = (torch.from_numpy(u).to(self.device), torch.from_numpy(s).to(self.device))
        return self._evals[key]

    def _batch_loaders(self, dataset, k=None):
        """nn/dcue.py:711-721: get_batches chunks, each a shuffled drop_last loader."""
        loaders = []
        for chunk in dataset.get_batches(k):
            it = _IndexBatches(chunk, self.batch_size)
            it.dataset = dataset
            loaders.append(it)
        return loaders

    # ------------------------------------------------------------------ fit
    def fit(self, train_dataset, val_dataset, test_dataset, pred_dataset, truth_dataset, item_dataset,
            n_users, n_items, triplets_path, metadata_path, save_dir, warm_start=False, audio_model=None):
        """nn/dcue.py:264-378 (same loop, same prints, same checkpoint policy)."""
        print("Settings:\n Feature Dim: {}\n Conv Dim: {}\n User Embedding Dim: {}\n Batch Size: {}\n "
              "Negative Batch Size: {}\n Margin: {}\n Optimizer: {}\n Learning Rate: {}\n Weight Decay: {}\n "
              "Restart Period: {}\n T Multiplier: {}\n Num Epochs: {}\n Model Type: {}\n Num Users: {}\n "
              "Num Items: {}\n Triplets TXT: {}\n Metadata CSV: {}\n Save Dir: {}".format(
                  self.feature_dim, self.conv_hidden, self.u_embdim, self.batch_size, self.neg_batch_size,
                  self.margin, self.optimize, self.lr, self.weight_decay, self.restart_period, self.t_mult,
                  self.num_epochs, self.model_type, n_users, n_items, triplets_path, metadata_path, save_dir),
              flush=True)
        if self.augment is not None:
            print(" Augment: {}".format(", ".join("%s=%s" % kv for kv in self.augment.items())), flush=True)
        self.epoch_size = int(int(np.ceil(len(train_dataset) / 10)) // self.batch_size) * self.batch_size
        self.n_users, self.n_items = n_users, n_items
        self.triplets_path, self.metadata_path = triplets_path, metadata_path
        self.model_dir = save_dir
        self.train_data, self.val_data, self.test_data = train_dataset, val_dataset, test_dataset
        self.pred_data, self.truth_data, self.item_data = pred_dataset, truth_dataset, item_dataset
        val_dataset.subset(p=self.val_pct)
        if not warm_start:
            self._init_nn(audio_model)
        self._bind_items(item_dataset)
        train_loss, samples_processed = 0, 0
        while self.nn_epoch < self.num_epochs + 1:
            for train_loader in self._batch_loaders(train_dataset, k=10):
                if self.nn_epoch > 0:
                    self.scheduler.step()
                    print("\nInitializing train epoch...", flush=True)
                    sp, train_loss = self._train_epoch(train_loader)
                    samples_processed += sp
                print("\nInitializing val epoch...", flush=True)
                _, val_loss = self._eval_epoch(val_dataset)
                print("\nInitializing AUC computation...", flush=True)
                self._user_factors(item_dataset)
                self._item_factors(item_dataset)
                val_auc, val_map = self._compute_scores('val', pred_dataset, truth_dataset, train_dataset,
                                                        val_dataset, test_dataset, pct=self.eval_pct)
                val_user_auc, val_user_map = self._compute_scores_song(pred_dataset, pct=self.eval_pct)
                train_auc, train_map = self._compute_scores('train', truth_dataset, truth_dataset, train_dataset,
                                                            val_dataset, test_dataset, pct=self.eval_pct)
                print("\nEpoch: [{}/{}]\tSamples: [{}/{}]\tTrain Loss: {}\tVal Loss: {}\tTrain AUC: {}\t"
                      "Val AUC: {}\tTrain mAP: {}\tVal mAP: {}\tVal UAUC: {}\tVal UmAP: {}".format(
                          self.nn_epoch, self.num_epochs, samples_processed, len(train_dataset) * self.num_epochs,
                          train_loss, val_loss, train_auc, val_auc, train_map, val_map, val_user_auc,
                          val_user_map), flush=True)
                self._update_best(val_map, val_auc, val_loss)
                self.nn_epoch += 1

    # ------------------------------------------------------------------ factors
    def _user_factors(self, item_data):
        """nn/dcue.py:629-638: eval user tower for every user index (one batched call)."""
        self.model.eval()
        self.model._require_device()
        self.user_factors = torch.zeros([self.n_users, self.feature_dim], device=self.device)
        idx = torch.as_tensor(np.fromiter(item_data.user_index.values(), dtype=np.int64)).to(self.device)
        step = 65536
        # the towers write rows at the storage width d_s (zero past d; include/dcue.h)
        ds = nat.storage_dims(self.model._flat["dims"]).feature_dim
        feat = torch.empty((min(step, max(idx.numel(), 1)), ds), device=self.device)
        model = self.model._model_struct()
        for s in range(0, idx.numel(), step):
            part = idx[s:s + step].contiguous()
            n = part.numel()
            ws = self._factor_ws(n, 1)
            nat.check(nat.lib().dcue_user_tower(ctypes.byref(model), nat.ptr(part), n, nat.ptr(ws), ws.numel(),
                                                nat.ptr(feat), nat.stream_handle()), "dcue_user_tower")
            self.user_factors.index_copy_(0, part, feat[:n, :self.feature_dim])

    def _factor_ws(self, rows, items):
        """Workspace of the factor passes, apart from the model's (a TrainPlan binds that one)."""
        nbytes = nat.workspace_bytes(self.model._flat["dims"], rows, 0, items)
        if getattr(self, "_fws", None) is None or self._fws.numel() < nbytes:
            self._fws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._fws

    def _item_factors(self, item_data, n_iter=10):
        """nn/dcue.py:640-668: [len(songid2metaindex), d], rows of the set's tracks = eval conv
        summed n_iter times / n_iter (identical passes for 131-frame tracks)."""
        self.item_factors = self._factors_over(item_data, n_iter)

    def get_item_factors(self, loader, n_iter=1):
        """nn/dcue.py:670-694."""
        return self._factors_over(_dataset(loader), n_iter)

    def _factors_over(self, item_data, n_iter):
        _loader_draws(n_iter)  # the reference iterates its item loader n_iter times
        self._bind_items(item_data)
        self.model.eval()
        self.model._require_device()
        n_meta = len(item_data.songid2metaindex)
        out = torch.zeros([n_meta, self.feature_dim], device=self.device)
        items = np.nonzero(self._item_meta >= 0)[0].astype(np.int32)
        if len(items) and self._store is not None:
            self._factors_cropped(items, int(n_iter), out)
        elif len(items):
            step = 8192
            ds = nat.storage_dims(self.model._flat["dims"]).feature_dim
            feat = torch.empty((min(step, len(items)), ds), device=self.device)
            tr = nat.Tracks(self._tracks.data_ptr(), self._tracks.shape[0],
                            0 if self._tracks.dtype == torch.float16 else 1, 0)
            model = self.model._model_struct()
            for s in range(0, len(items), step):
                it = torch.from_numpy(items[s:s + step]).to(self.device)
                n = it.numel()
                ws = self._factor_ws(1, n)
                nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(model), ctypes.byref(tr), nat.ptr(it), n,
                                                         nat.ptr(ws), ws.numel(), nat.ptr(feat), nat.stream_handle()),
                          "dcue_item_tower_eval")
                rows = torch.from_numpy(self._item_meta[items[s:s + step]]).to(self.device)
                out.index_copy_(0, rows, feat[:n, :self.feature_dim])
            nat.check(nat.lib().dcue_factor_repeat_mean(nat.ptr(out), out.numel(), int(n_iter), nat.stream_handle()),
                      "dcue_factor_repeat_mean")
        return out

    def _factor_crop(self, j, n_iter):
        """Window j of the n_iter an item factor averages over: 'random' draws 2^32 + j -- apart from
        every epoch's draw and the same each time, so factors stay comparable across epochs --, 'grid'
        the j-th of n_iter evenly spread windows."""
        if self.factor_crops == 'grid':
            return nat.crop_config(nat.CROP_GRID, grid_j=j, grid_n=n_iter)
        return nat.crop_config(nat.CROP_RANDOM, seed=self.crop_seed, draw=nat.CROP_FACTOR_DRAW0 + j)

    def _factors_cropped(self, items, n_iter, out):
        """nn/dcue.py:655-668 with a store bound: n_iter real passes. Per chunk of 8,192 items each
        pass cuts its windows into a scratch table through `rows` (the training table is never
        touched), runs the eval tower over it and adds the result in fp32, in pass order; one divide
        at the end -- the reference's `+=` then `/=`."""
        data, frame_ptr = self._store
        step = min(8192, len(items))
        ds = nat.storage_dims(self.model._flat["dims"]).feature_dim
        scratch = torch.empty((step, nat.N_FRAMES, nat.N_MELS), dtype=data.dtype, device=self.device)
        feat = torch.empty((step, ds), device=self.device)
        acc = torch.empty((step, self.feature_dim), device=self.device)
        ident = torch.arange(step, dtype=torch.int32, device=self.device)
        div = torch.tensor(float(n_iter), device=self.device)  # a device operand: a true fp32 division
        model = self.model._model_struct()
        for s in range(0, len(items), step):
            it = torch.from_numpy(items[s:s + step]).to(self.device)
            n = it.numel()
            tr = nat.Tracks(scratch.data_ptr(), n, 0 if scratch.dtype == torch.float16 else 1, 0)
            ws = self._factor_ws(1, n)
            acc.zero_()
            for j in range(n_iter):
                nat.crop_tracks(data, frame_ptr, self._factor_crop(j, n_iter), scratch[:n], rows=it)
                nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(model), ctypes.byref(tr), nat.ptr(ident), n,
                                                         nat.ptr(ws), ws.numel(), nat.ptr(feat), nat.stream_handle()),
                          "dcue_item_tower_eval")
                acc[:n] += feat[:n, :self.feature_dim]
            rows = torch.from_numpy(self._item_meta[items[s:s + step]]).to(self.device)
            out.index_copy_(0, rows, acc[:n] / div)

    def _item_feat_by_index(self):
        """item factors in item-index order (the evaluator's candidate rows)."""
        rows = torch.from_numpy(np.where(self._item_meta >= 0, self._item_meta, 0)).to(self.device)
        f = self.item_factors.index_select(0, rows)
        f[torch.from_numpy(self._item_meta < 0).to(self.device)] = 0
        return f

    # ------------------------------------------------------------------ scoring
    def _evaluator(self, kind, pred_ds, truth_ds=None):
        key = (kind, id(pred_ds), id(truth_ds))
        if key not in self._evals:
            inputs = (rank.user_split_inputs(pred_ds, truth_ds) if kind == "user" else rank.song_inputs(pred_ds))
            self._evals[key] = rank.RankEvaluator(inputs, self.device)
        return self._evals[key]

    def score_users(self, user_idx, pred_dataset, truth_dataset):
        """Per-user (auc, ap, has_pred_songs) arrays for user indices (the GPU core of score())."""
        ev = self._evaluator("user", pred_dataset, truth_dataset)
        return ev.metrics(self.user_factors, self._item_feat_by_index(), user_idx, nat.RANK_SPLIT)

    def score(self, users, pred_loader, truth_loader, k=10000):
        """nn/dcue.py:380-449: mean split-weighted AUC and mAP over `users` (user ids)."""
        self.model.eval()
        pred, truth = _dataset(pred_loader), _dataset(truth_loader)
        idx = np.array([pred.user_index[u] for u in users], dtype=np.int64)
        auc, ap, ok = self.score_users(idx, pred, truth)
        # torch-RNG parity: the reference iterates a shuffling loader per predict() call that finds
        # songs (base seed + sampler seed), for every user up to and including the one it stops at
        in_pred, in_truth = set(pred.triplets['user_id']), set(truth.triplets['user_id'])
        stop = int(np.argmin(ok)) + 1 if not ok.all() else len(users)
        _loader_draws(sum(2 * ((u in in_pred) + (u in in_truth)) for u in list(users)[:stop]))
        return rank.mean_until_missing(auc, ok), rank.mean_until_missing(ap, ok)

    def score_song(self, songs, pred_loader, k=10000):
        """nn/dcue.py:451-476: mean AUC and AP over `songs` (song ids); songs without users are
        skipped."""
        self.model.eval()
        pred = _dataset(pred_loader)
        idx = np.array([pred.item_index[s] for s in songs], dtype=np.int64)
        ev = self._evaluator("song", pred)
        auc, ap, ok = ev.metrics(self._item_feat_by_index(), self.user_factors, idx, nat.RANK_SINGLE)
        _loader_draws(2 * int(ok.sum()))  # one shuffling loader pass per song with users
        return float(np.mean(auc[ok])), float(np.mean(ap[ok]))

    def predict(self, user, loader):
        """nn/dcue.py:478-519: (scores, targets) over the user's pred-split candidate list, in the
        reference's order (the user's split triplets, then the other split songs by item index)."""
        ds = _dataset(loader)
        u = ds.user_index[user]
        pos = [ds.item_index[s] for s in ds.triplets.loc[ds.triplets['user_id'] == user, 'song_id']]
        if not pos:
            return None, None
        inter = set(ds.item_user.getcol(u).nonzero()[0].tolist())
        rest = [i for i in ds.split_items().tolist() if i not in inter]
        return self._sim_list(self.user_factors[u], pos + rest, [1] * len(pos) + [0] * len(rest), items=True)

    def predict_song(self, song, loader):
        """nn/dcue.py:521-562 (with the reference's non-user list: every split user but user 0)."""
        ds = _dataset(loader)
        i = ds.item_index[song]
        pos = [ds.user_index[x] for x in ds.triplets.loc[ds.triplets['song_id'] == song, 'user_id']]
        if not pos:
            return None, None
        rest = [u for u in ds.split_users().tolist() if u != 0]
        feat = self._item_feat_by_index()[i]
        return self._sim_list(feat, pos + rest, [1] * len(pos) + [0] * len(rest), items=False)

    def _sim_list(self, q, cands, targets, items):
        idx = torch.as_tensor(cands, dtype=torch.int64, device=self.device)
        rows = (self._item_feat_by_index() if items else self.user_factors).index_select(0, idx)
        with torch.no_grad():
            s = self.model.sim(q.unsqueeze(0).expand_as(rows), rows)
        return s.cpu().numpy().tolist(), [float(t) for t in targets]

    # ------------------------------------------------------------------ recommendation
    def _require_factors(self):
        if self.user_factors is None or self.item_factors is None or self._item_meta is None:
            raise RuntimeError("no factors to recommend from: fit the model (or call _user_factors / "
                               "_item_factors, or load a checkpoint and bind its item dataset) first")

    def _index_source(self, ds):
        """Whose user / item indices name the factor rows: every dataset of one triplets frame
        shares them (the category codes over all triplets)."""
        return ds if ds is not None else self.train_data if self.train_data is not None else self._tracks_src

    def _topk(self, kind, ds, exclude_seen, by_artist=False, with_artist=False):
        """rank.TopK per (kind, dataset, exclude_seen, by_artist, with_artist), cached as _evaluator caches
        its lists. by_artist: the exclusion rows also hold every song of the artists behind them
        (datasets.artists.artist_exclusion_csr) -- the artists a user has played, or a song's own artist.
        with_artist: only songs with a known artist are candidates."""
        if not (by_artist or with_artist):
            key = ("topk", kind, id(ds), bool(exclude_seen))
        else:
            key = ("topk", kind, id(ds), bool(exclude_seen), bool(by_artist), bool(with_artist))
        if key not in self._evals:
            mask = self._cand_mask(ds)
            if kind == "song":
                ptr, idx = rank.identity_csr(len(mask))
            elif exclude_seen or by_artist:
                src = ds if ds is not None else self.train_data
                if src is None:
                    raise RuntimeError("exclude_seen needs the interactions: pass dataset= (any split's "
                                       "dataset holds the all-split matrix) or fit() first")
                ptr, idx = src.user_item_csr()
            else:
                ptr = idx = None
            if by_artist or with_artist:
                group_of = self._artist_groups(ds)[0]
                if with_artist:
                    mask = mask & (group_of >= 0).astype(np.uint8)
                if by_artist:
                    ptr, idx = artist_exclusion_csr(group_of, played=None if kind == "song" else (ptr, idx),
                                                    seen=(ptr, idx) if kind == "song" or exclude_seen else None)
            self._evals[key] = rank.TopK(ptr, idx, mask, self.device)
        return self._evals[key]

    def set_artists(self, song_artist_map):
        """Who recorded each song: a {song_id: artist} dict (songs without an entry have no artist and are
        never capped), read by max_per_artist=, new_artists=, other_artists=, recommend_artists and
        evaluate_topk(artists=True). Without it the artists are those of the dataset in use, when that
        was built with song_artist_map. None forgets the artists."""
        self._song_artist_map = None if song_artist_map is None else dict(song_artist_map)
        for key in [k for k in self._evals if k[0] == "artists" or (k[0] == "topk" and len(k) > 4)]:
            del self._evals[key]

    def _artist_groups(self, ds):
        """(group_of int32 [n_items], artist names) over the item indices of ds (or the training data):
        datasets.artists.artist_groups, cached per index source."""
        src = self._index_source(ds)
        key = ("artists", id(src))
        if key not in self._evals:
            amap = self._song_artist_map if self._song_artist_map is not None else getattr(src, "song_artist_map", None)
            if amap is None:
                raise RuntimeError("no artists to go by: call set_artists({song_id: artist}) first, or use a "
                                   "dataset built with song_artist_map")
            self._evals[key] = artist_groups(src.item_index, amap)
        return self._evals[key]

    def set_popularity(self, counts=None, head_mass=_pop.HEAD_MASS):
        """How often each song is played: a {song_id: count} dict of non-negative integers (songs without an
        entry count 0), read by popularity= and evaluate_topk(novelty=True). None takes the training data's
        per-song user counts, the numbers neg_sampling='popularity' draws by. From the counts n_i over item
        indices (datasets.popularity, float64 on the host): z_i = log2(1 + n_i) / log2(1 + max n) in [0, 1],
        which popularity=beta scales into the serving prior float32(beta z_i); the self-information v_i =
        -log2((n_i + 1) / sum_j (n_j + 1)), whose mean over a list is its novelty; and the long-tail bytes --
        with the songs sorted by count descending (ties by index ascending) the head is the shortest prefix
        holding at least head_mass of all counts, everything else is tail."""
        self._popularity = ("train", float(head_mass)) if counts is None else (dict(counts), float(head_mass))
        for key in [k for k in self._evals if k[0] == "popularity"]:
            del self._evals[key]

    def _popularity_arrays(self, ds):
        """(z, self-information, tail bytes) over the item indices of ds (or the training data), cached per
        index source."""
        if self._popularity is None:
            raise RuntimeError("no play counts to go by: call set_popularity() first")
        src = self._index_source(ds)
        key = ("popularity", id(src))
        if key not in self._evals:
            counts, head_mass = self._popularity
            if isinstance(counts, str):
                data = src if hasattr(src, "item_user") else self.train_data
                if data is None:
                    raise RuntimeError("set_popularity() without counts needs the interactions: pass dataset= "
                                       "or fit() first")
                n = np.asarray(data.item_user.tocsr().getnnz(axis=1), dtype=np.int64)
            else:
                n = _pop.item_counts(src.item_index, counts)
            self._evals[key] = (_pop.log_popularity(n), _pop.self_information(n),
                                _pop.tail_bytes(n, head_mass))
        return self._evals[key]

    def _prior_kw(self, ds, popularity_, item_prior):
        """TopK.topk's prior argument for popularity= / item_prior= (neither: none, today's path). The array
        is cached per (index source, beta), so that TopK keeps its device copy between calls."""
        if popularity_ is not None and item_prior is not None:
            raise ValueError("popularity= and item_prior= both set: pass one prior")
        if item_prior is not None:
            return dict(prior=item_prior)
        if popularity_ is None:
            return {}
        beta = float(popularity_)
        if not np.isfinite(beta):
            raise ValueError("popularity must be finite, got %r" % (popularity_,))
        key = ("popularity", id(self._index_source(ds)), beta)
        if key not in self._evals:
            self._evals[key] = _pop.popularity_prior(self._popularity_arrays(ds)[0], beta)
        return dict(prior=self._evals[key])

    def _cap_kw(self, ds, max_per_artist, cap_rounds=4):
        """TopK.topk's group arguments for max_per_artist (None: none, today's path)."""
        if max_per_artist is None:
            return {}
        return dict(group_of=self._artist_groups(ds)[0], max_per_group=max_per_artist, cap_rounds=cap_rounds)

    def _as_pairs(self, ds, idx, score, count):
        names = self._index_source(ds).itemindex2songid
        return [[(names[int(i)], float(s)) for i, s in zip(idx[r, :count[r]], score[r, :count[r]])]
                for r in range(len(count))]

    def recommend(self, users, k=10, dataset=None, exclude_seen=True, as_ids=True, diversity=None, pool=None,
                  max_per_artist=None, new_artists=False, cap_rounds=4, popularity=None, item_prior=None):
        """The k best songs for each user id, by the cosine of DCUE.score: one list per user of
        (song_id, score) pairs, best first (as_ids=False: the raw (idx [n, k], score [n, k],
        count [n]) arrays over item indices). Candidates are the dataset's (or loader's) split songs,
        or every song with audio; exclude_seen drops the songs the user interacted with in any
        split -- the "seen" set of the evaluator's negatives. One fused GPU pass
        (include/dcue.h dcue_topk) for all users; the reference has only predict(), one user and one
        Python candidate list at a time. An unknown user id raises KeyError.

        diversity (lambda in [0, 1]; None: the plain ranking): the user's `pool` best songs (default
        min(128, 4 k)) re-ranked down to k by Maximal Marginal Relevance over the item factors' cosine
        (dcue_list_mmr): each pick maximises lambda * score - (1 - lambda) * (its largest similarity to
        the songs picked before it). The lists are then in selection order, each with its own score.

        max_per_artist (None: no cap; needs set_artists or a dataset with song_artist_map): no artist holds
        more than that many songs of a list (dcue_list_group_cap on the `pool` best songs; lists the cap
        leaves short are ranked deeper, at most cap_rounds - 1 times, and then equal the cap applied to
        the user's full ranking). A list can still come back shorter than k when the rounds or the
        catalogue run out. With diversity= the pool is capped before MMR picks from it. new_artists: the
        songs of every artist the user has played in any split are left out, played or not.

        popularity (beta; None: the plain cosine; needs set_popularity): every song's score gets the prior
        float32(beta z_i) added inside the fused ranking (dcue_topk_prior), z_i the song's scaled
        log-popularity in [0, 1] -- beta < 0 demotes the hits, beta > 0 promotes them, and the scores
        returned are the sums. item_prior: any finite array over item indices instead (boosts, recency, item
        biases); passing both raises ValueError. The prior reaches the pool of diversity= (whose relevance
        is then min-max scaled) and every round of max_per_artist=."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        index = self._index_source(ds).user_index
        rows = np.array([index[u] for u in users], dtype=np.int64)
        cap_kw = self._cap_kw(ds, max_per_artist, cap_rounds)
        cap_kw.update(self._prior_kw(ds, popularity, item_prior))
        out = self._topk("user", ds, exclude_seen, by_artist=new_artists).topk(
            self.user_factors, self._item_feat_by_index(), rows, k, diversity=diversity, pool=pool, **cap_kw)
        return self._as_pairs(ds, *out) if as_ids else out

    def recommend_artists(self, users, k=10, dataset=None, exclude_seen=True, new_artists=False, cap_rounds=4,
                          popularity=None, item_prior=None):
        """The k best ARTISTS for each user id: per user a list of (artist, best_song_id, score) triples,
        artists ranked by their best eligible song -- recommend(max_per_artist=1) over the songs with a
        known artist, mapped through the artists' names. Exact when no list comes back short of k (the
        deepening rounds, cap_rounds - 1 at the most, reached k artists or the end of the catalogue).
        exclude_seen / new_artists / popularity / item_prior: as recommend()."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        src = self._index_source(ds)
        group_of, names = self._artist_groups(ds)
        rows = np.array([src.user_index[u] for u in users], dtype=np.int64)
        idx, score, count = self._topk("user", ds, exclude_seen, by_artist=new_artists, with_artist=True).topk(
            self.user_factors, self._item_feat_by_index(), rows, k, **self._cap_kw(ds, 1, cap_rounds),
            **self._prior_kw(ds, popularity, item_prior))
        songs = src.itemindex2songid
        return [[(names[int(group_of[i])], songs[int(i)], float(s)) for i, s in zip(idx[r, :count[r]], score[r, :count[r]])]
                for r in range(len(count))]

    def _explained(self, tk, ds, query_feat, rows, k, reasons, diversity, pool, hist_ptr, hist_idx, as_ids,
                   cap_kw={}):
        """tk.topk's lists for `rows` plus dcue_list_explain's reasons over the history CSR, on the lists
        while they are on the device; the non-finite and bad-index checks of both calls."""
        feat = self._item_feat_by_index()
        idx, score, count, flags = tk.topk_raw(query_feat, feat, rows, k, diversity=diversity, pool=pool, **cap_kw)
        bad = (flags.cpu().numpy() & 2).astype(bool)
        if bad.any():
            raise tk._nonfinite(rows, bad)
        if "explain" not in self._evals:
            self._evals["explain"] = rank.Explain(self.device)
        why_idx, why_sim, eflags = self._evals["explain"].explain_raw(
            idx, count, rows, hist_ptr, hist_idx, feat, reasons, hist_mask=(self._item_meta >= 0).astype(np.uint8))
        rank.check_explain_flags(rows, eflags)
        idx, score, count = idx.cpu().numpy().astype(np.int64), score.cpu().numpy(), count.cpu().numpy()
        why_idx, why_sim = why_idx.cpu().numpy().astype(np.int64), why_sim.cpu().numpy()
        if not as_ids:
            return idx, score, count, why_idx, why_sim
        names = self._index_source(ds).itemindex2songid
        return [[(names[int(idx[r, j])], float(score[r, j]),
                  [(names[int(h)], float(s)) for h, s in zip(why_idx[r, j], why_sim[r, j]) if h >= 0])
                 for j in range(count[r])] for r in range(len(count))]

    def explain(self, users, k=10, reasons=3, dataset=None, exclude_seen=True, as_ids=True, diversity=None, pool=None,
                max_per_artist=None, new_artists=False, popularity=None, item_prior=None):
        """recommend()'s lists with the reason for every pick: per user a list of (song_id, score,
        [(history_song_id, similarity), ...]) triples -- the picks and scores are recommend()'s, bit for
        bit (the same dcue_topk call), and the `reasons` (1..8) history songs are those of the user's
        interactions in any split that have audio, by the cosine of the item factors: the score
        similar_songs reports for the pair (include/dcue.h dcue_list_explain, one launch on the device
        lists). A user without such a song gets empty reason lists. as_ids=False: the raw (idx [n, k],
        score [n, k], count [n], why_idx [n, k, reasons], why_sim [n, k, reasons]) arrays over item
        indices, short rows ending in -1 / -inf. diversity / pool / max_per_artist / new_artists / popularity /
        item_prior: as recommend() (the reasons' similarities stay plain cosines)."""
        reasons = rank.check_reasons(reasons)
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        src = self._index_source(ds)
        if not hasattr(src, "user_item_csr"):
            raise RuntimeError("explain needs the interactions: pass dataset= (any split's dataset holds the "
                               "all-split matrix) or fit() first")
        rows = np.array([src.user_index[u] for u in users], dtype=np.int64)
        tk = self._topk("user", ds, exclude_seen, by_artist=new_artists)
        if exclude_seen and not new_artists and src is (ds if ds is not None else self.train_data):
            hist = (tk.excl_ptr, tk.excl_idx)  # the CSR _topk already uploaded
        else:
            key = ("history", id(src))
            if key not in self._evals:
                self._evals[key] = rank._upload_csr(*src.user_item_csr(), self.device)
            hist = self._evals[key]
        return self._explained(tk, ds, self.user_factors, rows, k, reasons, diversity, pool, *hist, as_ids,
                               dict(self._cap_kw(ds, max_per_artist), **self._prior_kw(ds, popularity, item_prior)))

    def similar_songs(self, songs, k=10, dataset=None, max_per_artist=None, other_artists=False, pool=None):
        """The k songs most similar to each song id (item-to-item on the same kernel: the item factors
        on both sides, each song excluded from its own list); same return as recommend().
        max_per_artist / pool: as recommend(). other_artists: no song by the query song's own artist is
        returned ("similar songs, but not by the same artist")."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        index = self._index_source(ds).item_index
        rows = np.array([index[s] for s in songs], dtype=np.int64)
        feat = self._item_feat_by_index()
        return self._as_pairs(ds, *self._topk("song", ds, True, by_artist=other_artists).topk(
            feat, feat, rows, k, pool=pool, **self._cap_kw(ds, max_per_artist)))

    # ------------------------------------------------------------------ unseen songs
    def embed_audio(self, wave, logmel=None, frame0=0, crops=None, sample_rate=None, resample="best"):
        """[n, d] item factors of waveforms ([n_samples] or [n, n_samples], mono, at the front end's
        sample rate, or at sample_rate when one is given: the clips are then resampled on the GPU first,
        audio.Resampler with quality `resample`, and frame0 counts frames of the resampled clip) -- the cold-start step for a song nobody has played: audio.LogMel.track_rows writes
        a temporary fp16 track table on the GPU (frames frame0 .. frame0 + 130 of each clip) and
        dcue_item_tower_eval reads it where it lies. Needs no dataset and no host copy. logmel: an
        audio.LogMel (default: one with the default configuration, kept for later calls). A clip with a
        NaN or infinite sample raises ValueError naming it.

        crops=n embeds the whole clip instead of one window: the front end runs over every frame, the
        rows become a uniform track store, and the factor is the fp32 mean, in window order, of the
        tower over n evenly spread 131-frame windows (dcue_crop_tracks, DCUE_CROP_GRID: the first starts
        at frame 0, the last ends at the clip's last frame; n = 1 is the centre window). A clip shorter
        than 131 frames raises ValueError, as a frame0 past the end does."""
        from dcrecommend import audio
        if self.model._flat["dims"].tower == nat.TOWERS[nat.TEXT_TOWER]:
            raise RuntimeError("embed_audio: the text tower needs a song's tokens too; audio alone is not enough")
        if logmel is None:
            if getattr(self, "_logmel", None) is None:
                self._logmel = audio.LogMel(device=self.device)
            logmel = self._logmel
        self.model.eval()
        self.model._require_device()
        ds = nat.storage_dims(self.model._flat["dims"]).feature_dim
        if sample_rate is not None:
            wave = logmel._at_rate(wave, sample_rate, resample)
        if crops is None:
            return self._tower_over(logmel.track_rows(wave, frame0, torch.float16), ds)[:, :self.feature_dim].contiguous()
        crops = int(crops)
        if crops < 1 or frame0 != 0:
            raise ValueError("embed_audio: crops must be >= 1 and goes without frame0")
        rows = logmel.transform(wave, 0, None, torch.float16)  # every frame of every clip
        n, T = int(rows.shape[0]), int(rows.shape[1])
        if T < nat.N_FRAMES:
            raise ValueError("embed_audio: crops needs clips of at least %d frames; the frame range of these "
                             "clips ends at %d (no silent padding)" % (nat.N_FRAMES, T))
        acc = torch.zeros((n, self.feature_dim), device=self.device)
        if n:
            frame_ptr = torch.arange(n + 1, dtype=torch.int64, device=self.device) * T
            table = torch.empty((n, nat.N_FRAMES, nat.N_MELS), dtype=torch.float16, device=self.device)
            for j in range(crops):
                nat.crop_tracks(rows.view(n * T, nat.N_MELS), frame_ptr,
                                nat.crop_config(nat.CROP_GRID, grid_j=j, grid_n=crops), table)
                acc += self._tower_over(table, ds)[:, :self.feature_dim]
        return acc / torch.tensor(float(crops), device=self.device)

    def _tower_over(self, table, ds):
        """dcue_item_tower_eval over every row of a temporary track table: [n, d_s] features."""
        n = int(table.shape[0])
        feat = torch.empty((max(n, 1), ds), device=self.device)
        if n:
            tr = nat.Tracks(table.data_ptr(), n, 0 if table.dtype == torch.float16 else 1, 0)
            it = torch.arange(n, dtype=torch.int32, device=self.device)
            model = self.model._model_struct()
            ws = self._factor_ws(1, n)
            nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(model), ctypes.byref(tr), nat.ptr(it), n,
                                                     nat.ptr(ws), ws.numel(), nat.ptr(feat), nat.stream_handle()),
                      "dcue_item_tower_eval")
        return feat[:n]

    def similar_to_audio(self, wave, k=10, dataset=None, logmel=None, crops=None, sample_rate=None, resample="best",
                         max_per_artist=None, other_artists=False):
        """The k catalogue songs nearest to each clip, by the cosine of its embed_audio factor to the
        item factors: one list of (song_id, score) pairs per clip, as similar_songs returns (nothing is
        excluded: the clip is not in the catalogue). crops: as embed_audio -- the whole song, not its
        first window. sample_rate / resample: as embed_audio. max_per_artist: as recommend().
        other_artists: False, or one artist name per clip (None: no artist) -- the clip's own artist, whose
        catalogue songs are then left out of its list."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        q = self.embed_audio(wave, logmel, crops=crops, sample_rate=sample_rate, resample=resample)
        tk = self._topk("audio", ds, False)
        if other_artists is not False:
            group_of, names = self._artist_groups(ds)
            own = list(other_artists)
            if len(own) != q.shape[0]:
                raise ValueError("other_artists names %d artists for %d clips" % (len(own), q.shape[0]))
            tk = rank.TopK(*rank.histories_csr([np.flatnonzero(group_of == names.index(a)) if a in names else []
                                                for a in own]), self._cand_mask(ds), self.device)
        out = tk.topk(q, self._item_feat_by_index(), np.arange(q.shape[0]), k, **self._cap_kw(ds, max_per_artist))
        return self._as_pairs(ds, *out)

    def listeners_for_audio(self, wave, k=10, logmel=None, crops=None, sample_rate=None, resample="best"):
        """The k users with the highest cosine to each clip -- "who should hear this": the clips'
        embed_audio factors against user_factors on the same kernel. One list of (user_id, score) pairs
        per clip, best first. crops, sample_rate, resample: as embed_audio."""
        self._require_factors()
        q = self.embed_audio(wave, logmel, crops=crops, sample_rate=sample_rate, resample=resample)
        key = ("topk", "listeners")
        if key not in self._evals:
            self._evals[key] = rank.TopK(None, None, None, self.device, n_cand=int(self.user_factors.shape[0]))
        idx, score, count = self._evals[key].topk(q, self.user_factors, np.arange(q.shape[0]), k)
        names = self._index_source(None).userindex2userid
        return [[(names[int(i)], float(s)) for i, s in zip(idx[r, :count[r]], score[r, :count[r]])]
                for r in range(len(count))]

    # ------------------------------------------------------------------ list quality
    def _topk_metrics(self, ds):
        """rank.TopKMetrics per dataset, cached as _topk caches its lists, and the user rows with a
        non-empty truth row. Truth = the all-split interaction row restricted to the candidates."""
        key = ("topk_metrics", id(ds))
        if key not in self._evals:
            mask = self._cand_mask(ds)
            src = ds if ds is not None else self.train_data
            if src is None:
                raise RuntimeError("evaluate_topk needs the interactions: pass dataset= (any split's "
                                   "dataset holds the all-split matrix) or fit() first")
            ptr, idx = src.user_item_csr()
            keep = mask[idx] != 0
            kept = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
            ptr, idx = kept[ptr], idx[keep]
            self._evals[key] = (rank.TopKMetrics(ptr, idx, self.device, cand_mask=mask),
                                np.flatnonzero(np.diff(ptr) > 0).astype(np.int64))
        return self._evals[key]

    def evaluate_topk(self, dataset=None, ks=(10, 50, 100), users=None, per_user=False, diversity=None, pool=None,
                      ild=False, artists=False, max_per_artist=None, popularity=None, item_prior=None, novelty=False):
        """Top-K ranking quality of the current factors: {"precision@K", "recall@K", "ndcg@K", "map@K",
        "mrr@K", "hit@K", "coverage@K" for each K of ks, "n_users"} (include/dcue.h dcue_topk_metrics
        has the definitions). Candidates are the dataset's (or loader's) split songs with audio, or
        every song with audio; a user's truth is every candidate the user interacted with in any
        split -- with a song-split dataset the held-out songs, none of which training saw. users:
        user ids (an unknown one raises KeyError); default every user with a non-empty truth row, in
        index order. Users without truth are left out of the means; n_users counts the others.
        per_user adds "users" (the ids), "per_user" (numpy [n, len(ks), 6], slots in
        _native.TOPK_METRIC_NAMES order) and "flags" (bit 0: no truth). Every list is ranked and
        scored on the GPU (dcue_topk, then dcue_topk_metrics on its device output); the reference has
        only DCUE.score's sampled AUC / mAP.

        diversity / pool: score recommend(diversity=, pool=)'s MMR re-ranked lists (k = max(ks)) instead.
        ild adds "ild@K" -- the mean intra-list diversity (1 - cosine of the item factors, averaged
        over the pairs of a list's first K songs; dcue_list_ild) of the lists that were scored -- and
        "n_ild", the number of lists behind it.

        max_per_artist: score recommend(max_per_artist=)'s capped lists. artists adds "artists@K" (the mean
        number of distinct artists among a list's first K songs, a song without an artist counting as one
        of its own), "artist_top@K" (the mean of the most songs one artist holds there) and
        "artist_coverage@K" (the share of the artists with a candidate song that appear in some list's
        first K), by dcue_list_group_stats on the same device lists, and "n_artist_lists".

        popularity / item_prior: score recommend(popularity=) / recommend(item_prior=)'s lists, the ones that
        would be served. novelty (needs set_popularity) adds "novelty@K" (the mean over the lists of the
        first K songs' mean self-information, in bits: higher = further from the hits), "tail@K" (the mean
        share of long-tail songs among them), both by dcue_list_item_stats on the same device lists, with
        "n_novelty" the lists behind them, and "gini@K" (the Gini index of the candidates' exposure in the
        lists' first K entries: 0 = all served equally often; dcue_exposure_gini)."""
        ks = rank.check_cutoffs(ks)
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        src = self._index_source(ds)
        ev, with_truth = self._topk_metrics(ds)
        if users is None:
            rows = with_truth
            users = [src.userindex2userid[int(r)] for r in rows] if per_user else None
        else:
            users = list(users)
            rows = np.array([src.user_index[u] for u in users], dtype=np.int64)
        cap_kw = self._cap_kw(ds, max_per_artist)
        if artists:
            cap_kw.update(group_of=self._artist_groups(ds)[0], group_stats=True)
        cap_kw.update(self._prior_kw(ds, popularity, item_prior))
        if novelty:
            _, value, tail = self._popularity_arrays(ds)
            cap_kw.update(item_value=value, item_tail=tail, gini=True)
        res = ev.evaluate(self.user_factors, self._item_feat_by_index(), rows, ks, per_query=per_user,
                          diversity=diversity, pool=pool, ild=ild, **cap_kw)
        out = {"n_users": res["n_evaluated"]}
        for name in nat.TOPK_METRIC_NAMES + ("coverage",) + (("ild",) if ild else ()):
            for i, k in enumerate(ks):
                out["%s@%d" % (name, k)] = float(res[name][i])
        if artists:
            for name, slot in (("artists", "group_distinct"), ("artist_top", "group_top"),
                               ("artist_coverage", "group_coverage")):
                for i, k in enumerate(ks):
                    out["%s@%d" % (name, k)] = float(res[slot][i])
            out["n_artist_lists"] = res["n_group"]
        if ild:
            out["n_ild"] = res["n_ild"]
        if novelty:
            for name in ("novelty", "tail", "gini"):
                for i, k in enumerate(ks):
                    out["%s@%d" % (name, k)] = float(res[name][i])
            out["n_novelty"] = res["n_novelty"]
        if per_user:
            out.update(users=users, per_user=res["per_query"], flags=res["flags"])
        return out

    # ------------------------------------------------------------------ unseen users
    def _cand_mask(self, ds):
        """The candidates of _topk: songs with audio (the others have zero factors), in the split."""
        mask = (self._item_meta >= 0).astype(np.uint8)
        if ds is not None:
            split = np.zeros_like(mask)
            split[ds.split_items()] = 1
            mask &= split
        return mask

    def _history_items(self, histories, ds):
        """(usable, full): per history the item indices with audio, and all of them. An unknown song
        id raises KeyError, a history without a usable song ValueError."""
        index = self._index_source(ds).item_index
        usable, full = [], []
        for h, songs in enumerate(histories):
            items = sorted({int(index[s]) for s in songs})
            full.append(items)
            usable.append([i for i in items if self._item_meta[i] >= 0])
            if not usable[-1]:
                raise ValueError("history %d has no song with audio: nothing to fold in from" % h)
        return usable, full

    def fold_in(self, histories, steps=30, n_neg=None, lr=None, max_pos=64, seed=0, dataset=None, init=None):
        """User factors [n, feature_dim] (device) for users outside the trained table -- a new
        listener, a playlist, a session -- each given as a list of song ids. With the model frozen,
        one fresh embedding row per history is learned against the trained towers with the training
        loss itself (cosine hinge, n_neg sampled negatives per positive, Adam on that row only; margin,
        betas and eps are the trainer's, n_neg defaults to neg_batch_size and lr to the trainer's): all
        steps of all users in one kernel launch (include/dcue.h dcue_user_foldin). The reference has no
        counterpart: its predict() looks the user up in user_index.

        init [n, u_embdim]: the rows' starting values; default N(0, 1) rows from a CPU torch.Generator
        seeded with `seed` (nn.Embedding's distribution). Songs without audio are dropped from the
        positives. An unknown song id raises KeyError, a history with no usable song ValueError."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        usable, _ = self._history_items(histories, ds)
        return self._fold_in(usable, ds, steps, n_neg, lr, max_pos, seed, init)[1]

    def _fold_in(self, usable, ds, steps, n_neg, lr, max_pos, seed, init):
        self.model._require_device()
        n = len(usable)
        if init is None:
            gen = torch.Generator().manual_seed(int(seed))
            init = torch.randn(n, self.u_embdim, generator=gen)
        init = torch.as_tensor(init, dtype=torch.float32).to(self.device)
        key = ("foldin", id(ds))
        if key not in self._evals:
            self._evals[key] = rank.FoldIn(self._cand_mask(ds), self.device)
        cfg = rank.FoldIn.config(steps, self.neg_batch_size if n_neg is None else n_neg, max_pos, self.margin,
                                 self.lr if lr is None else lr, self.beta_one, self.beta_two, self.eps, 0.0, seed)
        ptr, idx = rank.histories_csr(usable)
        emb, feat, loss, _, flags = self._evals[key].fold_in_raw(self.model._model_struct(),
                                                                 self._item_feat_by_index(), ptr, idx, init, cfg)
        bad = (flags.cpu().numpy() & nat.FOLDIN_NONFINITE).astype(bool)
        if bad.any():
            raise ValueError("Input contains NaN. (fold-in of history %d: the loss or the factor is not "
                             "finite)" % int(np.argmax(bad)))
        return emb, feat, loss

    def recommend_for(self, histories, k=10, dataset=None, exclude_history=True, as_ids=True, diversity=None,
                      pool=None, max_per_artist=None, new_artists=False, popularity=None, item_prior=None,
                      **fold_in_kwargs):
        """recommend() for users outside the trained table: fold_in(histories, **fold_in_kwargs), then
        the fused top-k pass with each history as the user's exclusion list (every song of it, with
        or without audio). diversity / pool / max_per_artist: as recommend(); new_artists: the songs of
        every artist in the history are left out; popularity / item_prior: as recommend(). Returns what
        recommend() returns."""
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        usable, full = self._history_items(histories, ds)
        args = dict(steps=30, n_neg=None, lr=None, max_pos=64, seed=0, init=None)
        unknown = set(fold_in_kwargs) - set(args)
        if unknown:
            raise TypeError("recommend_for() got unexpected fold_in arguments %s" % sorted(unknown))
        args.update(fold_in_kwargs)
        feat = self._fold_in(usable, ds, **args)[1]
        ptr, idx = self._history_exclusion(ds, full, exclude_history, new_artists)
        out = rank.TopK(ptr, idx, self._cand_mask(ds), self.device).topk(
            feat, self._item_feat_by_index(), np.arange(len(full)), k, diversity=diversity, pool=pool,
            **self._cap_kw(ds, max_per_artist), **self._prior_kw(ds, popularity, item_prior))
        return self._as_pairs(ds, *out) if as_ids else out

    def _history_exclusion(self, ds, full, exclude_history, new_artists):
        """The exclusion CSR of recommend_for / explain_for: the histories, and with new_artists every
        song of their artists; (None, None) for neither."""
        hist = rank.histories_csr(full)
        if new_artists:
            return artist_exclusion_csr(self._artist_groups(ds)[0], played=hist, seen=hist if exclude_history else None)
        return hist if exclude_history else (None, None)

    def explain_for(self, histories, k=10, reasons=3, dataset=None, exclude_history=True, as_ids=True, diversity=None,
                    pool=None, max_per_artist=None, new_artists=False, popularity=None, item_prior=None,
                    **fold_in_kwargs):
        """recommend_for() with the reason for every pick: the lists are recommend_for()'s (the same
        fold-in and dcue_topk calls), the reasons the `reasons` (1..8) songs of each given history that
        have audio, nearest to the pick by the cosine of the item factors. Returns what explain() returns."""
        reasons = rank.check_reasons(reasons)
        self._require_factors()
        ds = None if dataset is None else _dataset(dataset)
        usable, full = self._history_items(histories, ds)
        args = dict(steps=30, n_neg=None, lr=None, max_pos=64, seed=0, init=None)
        unknown = set(fold_in_kwargs) - set(args)
        if unknown:
            raise TypeError("explain_for() got unexpected fold_in arguments %s" % sorted(unknown))
        args.update(fold_in_kwargs)
        feat = self._fold_in(usable, ds, **args)[1]
        ptr, idx = self._history_exclusion(ds, full, exclude_history, new_artists)
        tk = rank.TopK(ptr, idx, self._cand_mask(ds), self.device)
        return self._explained(tk, ds, feat, np.arange(len(full)), k, reasons, diversity, pool,
                               *rank.histories_csr(usable), as_ids,
                               dict(self._cap_kw(ds, max_per_artist), **self._prior_kw(ds, popularity, item_prior)))

    def _compute_scores(self, split, pred_loader, truth_loader, train_data, val_data, test_data, pct=0.025):
        """nn/dcue.py:580-603."""
        if split == 'train':
            users = list(train_data.uniq_users)
        elif split == 'val':
            users = list(set(train_data.uniq_users).intersection(set(val_data.uniq_users)))
        elif split == 'test':
            users = list(set(train_data.uniq_users).intersection(set(test_data.uniq_users)))
        else:
            raise ValueError(split)
        sample = np.random.choice(users, int(len(users) * pct)) if pct < 1 else users
        return self.score(sample, pred_loader, truth_loader)

    def _compute_scores_song(self, pred_loader, pct=0.025):
        """nn/dcue.py:605-613."""
        songs = list(_dataset(pred_loader).uniq_songs)
        sample = np.random.choice(songs, int(len(songs) * pct)) if pct < 1 else songs
        return self.score_song(sample, pred_loader)

    # ------------------------------------------------------------------ bookkeeping
    def insert_best_factors(self):
        self.item_factors = self.best_item_factors
        self.user_factors = self.best_user_factors

    def _update_best(self, val_map, val_auc, val_loss):
        """nn/dcue.py:564-578: keep the best-by-val-mAP factors; checkpoint then, or every 5th."""
        if val_map > self.best_val_map:
            self.best_val_map, self.best_val_auc, self.best_val_loss = val_map, val_auc, val_loss
            if self.best_item_factors is None or self.best_user_factors is None:
                self.best_item_factors = torch.zeros_like(self.item_factors)
                self.best_user_factors = torch.zeros_like(self.user_factors)
            self.best_item_factors.copy_(self.item_factors)
            self.best_user_factors.copy_(self.user_factors)
            self.save(models_dir=self.model_dir)
        elif self.nn_epoch % 5 == 0:
            self.save(models_dir=self.model_dir)

    def _format_model_subdir(self):
        return ("DCUE_fd_{}_ch_{}_uh_{}_op_{}_lr_{}_wd_{}_rp_{}_tm_{}_nu_{}_ni_{}_mt_{}".format(
            self.feature_dim, self.conv_hidden, self.u_embdim, self.optimize, self.lr, self.weight_decay,
            self.restart_period, self.t_mult, self.n_users, self.n_items, self.model_type))

    _SCALARS = ("feature_dim", "conv_hidden", "batch_size", "neg_batch_size", "u_embdim", "margin", "optimize",
                "lr", "beta_one", "beta_two", "eps", "weight_decay", "restart_period", "t_mult", "num_epochs",
                "model_type", "eval_pct", "val_pct", "n_users", "n_items", "epoch_size", "nn_epoch",
                "best_val_map", "best_val_auc", "best_val_loss", "metadata_path", "triplets_path", "model_dir",
                "defer_embedding", "crop", "crop_seed", "factor_crops", "neg_pool", "neg_hard", "augment")
    _TENSORS = ("item_factors", "user_factors", "best_item_factors", "best_user_factors")

    def _checkpoint(self):
        out = {k: getattr(self, k) for k in self._SCALARS}
        out.update({k: (None if getattr(self, k) is None else getattr(self, k).cpu()) for k in self._TENSORS})
        out["model"] = {k: v.cpu() for k, v in self.model.state_dict().items()}
        opt = self.optimizer.state_dict()
        mom = opt["native"]["moments"]
        out["optimizer"] = {"step": opt["native"]["step"],
                            "moments": None if mom is None else {k: v.cpu() for k, v in mom.items()}}
        out["scheduler"] = {k: v for k, v in self.scheduler.__dict__.items()
                            if isinstance(v, (int, float, bool, str)) or v is None}
        return out

    def save(self, models_dir=None):
        """nn/dcue.py:723-741: models_dir/<subdir>/epoch_{n}.pth. The file holds tensors and plain
        values only (torch.load(weights_only=True) reads it); the reference pickles the trainer."""
        if self.model is None or models_dir is None:
            return
        d = os.path.join(models_dir, self._format_model_subdir())
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "epoch_{}.pth".format(self.nn_epoch)), 'wb') as f:
            torch.save(self._checkpoint(), f)

    def load(self, model_dir, epoch):
        """nn/dcue.py:743-785: restore attributes, model, optimizer and scheduler; nn_epoch + 1."""
        with open(os.path.join(model_dir, "epoch_{}.pth".format(epoch)), 'rb') as f:
            ck = torch.load(f, map_location="cpu", weights_only=True)
        for k in self._SCALARS:
            if k in ck:
                setattr(self, k, ck[k])
        if "crop" not in ck:  # a checkpoint from before the per-epoch crops: the table cut once, at load
            self.crop, self.crop_seed, self.factor_crops = 'load', 0, 'random'
        if "augment" not in ck or self.crop != 'epoch':  # a checkpoint from before the augmentation: none
            self.augment = None
        self._init_nn()
        self.model.load_state_dict(ck["model"])
        for k in self._TENSORS:
            setattr(self, k, None if ck.get(k) is None else ck[k].to(self.device))
        opt = ck["optimizer"]
        moments = None if opt["moments"] is None else {k: v.to(self.device) for k, v in opt["moments"].items()}
        base = self.optimizer.state_dict()
        base["native"] = dict(step=opt["step"], moments=moments)
        self.optimizer.load_state_dict(base)
        self.scheduler.__dict__.update(ck["scheduler"])
        self.nn_epoch += 1
