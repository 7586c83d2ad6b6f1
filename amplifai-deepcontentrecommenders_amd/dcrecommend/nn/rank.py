"""GPU ranking evaluation of DCUE (nn/dcue.py:380-476) over include/dcue.h dcue_rank_metrics.

The reference scores one user at a time: it builds a pandas frame of every split song
(DCUEPredset.create_user_data), batches it through a DataLoader, gathers factors row by row,
calls model.sim and sklearn's roc_auc_score / average_precision_score. Here the candidate lists
are two bitmasks over the catalogue plus the all-split interaction CSR, built once per dataset on
the host, and every sampled query is ranked on the GPU in one call.

TopK (dcue_topk) is the serving counterpart: the k best candidates per query, with a candidate mask
and a per-query exclusion CSR, fused so that the score matrix is never written.

TopKMetrics (dcue_topk_metrics) says how good TopK's lists are: Precision / Recall / NDCG / MAP / MRR /
HitRate at several cutoffs and catalogue coverage against held-out truth rows, on the device lists.

Diversify (dcue_list_mmr / dcue_list_ild) trades relevance against redundancy: Maximal Marginal Relevance
re-ranking of TopK's device lists, and their intra-list diversity next to TopKMetrics' numbers.

Explain (dcue_list_explain) says why a song is in a list: for every pick, the songs of the user's
history nearest to it by the cosine similar_songs reports, on the same device lists.

GroupCap (dcue_list_group_cap / dcue_list_group_stats) knows who made a song: at most so many entries per
group (artist, album, label) of TopK's device lists, and how many groups a list spans.

TopK's prior= (dcue_topk_prior) adds a per-candidate term to every score inside the fused ranking --
popularity promotion or demotion, boosts, item biases -- and PopStats (dcue_list_item_stats /
dcue_exposure_gini) says where the lists sit on that trade-off: novelty, long-tail share, exposure Gini.

FoldIn (dcue_user_foldin) gives users outside the trained table a factor: one embedding row per user
learned against the frozen towers, all steps in one kernel launch.
"""
import ctypes

import numpy as np
import torch

from dcrecommend import _native as nat

LIST_PRED, LIST_TRUTH = 1, 2


def _csr_users_to_items(ds):
    csc = ds.item_user.tocsc()  # columns = users
    csc.sort_indices()
    return csc.indptr.astype(np.int64), csc.indices.astype(np.int32)


def _csr_items_to_users(ds):
    csr = ds.item_user.tocsr()  # rows = items
    csr.sort_indices()
    return csr.indptr.astype(np.int64), csr.indices.astype(np.int32)


def user_split_inputs(pred_ds, truth_ds, index_ds=None):
    """DCUE.score's candidate lists (nn/dcue.py:399-416 over dcuepredset.py:39-93): pred list =
    the pred split's songs, truth list = the truth split's songs, a user's positives = every song
    the user interacted with in any split (the lists' negatives exclude all of them)."""
    index_ds = index_ds if index_ds is not None else pred_ds
    ptr, idx = _csr_users_to_items(index_ds)
    cls = np.zeros(index_ds.n_items, dtype=np.uint8)
    cls[pred_ds.split_items()] |= LIST_PRED
    cls[truth_ds.split_items()] |= LIST_TRUTH
    return {"pos_ptr": ptr, "pos_idx": idx, "cand_class": cls}


def song_inputs(pred_ds):
    """DCUE.score_song's lists (nn/dcue.py:463-474 over dcuepredset.py:53-62, 95-124): positives =
    the song's users (bit 1 = the split's users); label-0 list (bit 0) = every split user except
    user index 0, the song's own users included -- the reference's `getrow(i).nonzero()[0]` yields
    row indices (all 0), so only user 0 is ever excluded."""
    ptr, idx = _csr_items_to_users(pred_ds)
    cls = np.zeros(pred_ds.n_users, dtype=np.uint8)
    users = pred_ds.split_users()
    cls[users] = LIST_PRED | LIST_TRUTH
    if len(pred_ds.split_items()):
        cls[0] &= ~np.uint8(LIST_PRED)
    return {"pos_ptr": ptr, "pos_idx": idx, "cand_class": cls}


def mean_until_missing(values, has_pos):
    """DCUE.score's mean: the user loop `break`s at the first user without pred-split songs
    (nn/dcue.py:393-394), so only the users before it count."""
    has_pos = np.asarray(has_pos, bool)
    stop = int(np.argmin(has_pos)) if not has_pos.all() else len(has_pos)
    return float(np.mean(np.asarray(values, np.float64)[:stop]))


def _upload_csr(ptr, idx, device):
    """(int64 pointers, int32 indices) on the device; an empty index array becomes one unused entry,
    so that its address is never null. Tensors (a CSR already on a device) are taken as they are."""
    if torch.is_tensor(ptr):
        idx = idx if idx.numel() else torch.zeros(1, dtype=torch.int32)
        return ptr.to(device, torch.int64).contiguous(), idx.to(device, torch.int32).contiguous()
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    return (torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(device),
            torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(device))


def _upload_mask(cand_mask, n_cand, device):
    """(uint8 mask on the device, its length), or (None, n_cand) without a mask."""
    if torch.is_tensor(cand_mask):  # (a mask already on a device)
        mask = cand_mask.to(device, torch.uint8).contiguous()
        return mask, int(mask.numel())
    if cand_mask is not None:
        mask = torch.from_numpy(np.ascontiguousarray(cand_mask, dtype=np.uint8)).to(device)
        return mask, int(mask.numel())
    if n_cand is None:
        raise ValueError("n_cand is needed without a candidate mask")
    return None, int(n_cand)


def _check_shapes(cand_feat, n_cand, d, query_feat=None, ptr=None):
    """The candidate factors are [n_cand, d]; the query factors have one row per CSR row."""
    if cand_feat.shape[0] != n_cand or cand_feat.shape[1] != d:
        raise ValueError("candidate factors %s do not match %d candidates / d=%d" % (tuple(cand_feat.shape), n_cand, d))
    if ptr is not None and query_feat.shape[0] + 1 != ptr.numel():
        raise ValueError("query factors have %d rows, the CSR %d" % (query_feat.shape[0], ptr.numel() - 1))


def _nonfinite_error(queries, bad):
    """sklearn's wording for the first query of `bad` (a cosine of finite factors is finite:
    non-finite factors make NaN scores)."""
    return ValueError("Input contains NaN. (DCUE scores of query %d: the model's factors are not "
                      "finite)" % int(np.asarray(queries).reshape(-1)[int(np.argmax(bad))]))


def _nonfinite_dot_error(queries, bad):
    """The same for inner-product scores, which finite factors can overflow."""
    return ValueError("Input contains NaN or infinity. (inner-product scores of query %d: the factors are not "
                      "finite or the product overflowed)" % int(np.asarray(queries).reshape(-1)[int(np.argmax(bad))]))


def _score_mode(score):
    if score not in nat.SCORES:
        raise ValueError("score must be one of %s, got %r" % (sorted(nat.SCORES), score))
    return nat.SCORES[score]


class _Workspace:
    """The grow-only device workspace of one entry point, sized by its dcue_*_workspace_bytes."""

    _ws = None

    def _nbytes(self, name, *args):
        nbytes = ctypes.c_size_t()
        nat.check(getattr(nat.lib(), name)(*args, ctypes.byref(nbytes)), name)
        return nbytes.value

    def _grow(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws


class RankEvaluator(_Workspace):
    """Device-resident candidate lists for one (query kind, pred split, truth split) and the
    workspace of dcue_rank_metrics."""

    def __init__(self, inputs, device, max_score_bytes=1 << 30):
        self.device = torch.device(device)
        self.pos_ptr, self.pos_idx = _upload_csr(inputs["pos_ptr"], inputs["pos_idx"], self.device)
        self.cand_class, self.n_cand = _upload_mask(inputs["cand_class"], None, self.device)
        self.max_score_bytes = max_score_bytes

    def metrics(self, query_feat, cand_feat, queries, mode):
        """(auc, ap, has_pos) numpy arrays, one entry per query (fp64).

        Raises ValueError where the reference's sklearn calls would (roc_auc_score /
        average_precision_score on NaN or infinite scores, nn/dcue.py:440,447,473-474): DCUE.score
        for a query before the first one without pred positives (its loop breaks there, :396-397),
        DCUE.score_song for any query with both labels."""
        nat.require_gpu(query_feat, "query_feat")
        nat.require_gpu(cand_feat, "cand_feat")
        query_feat = query_feat.contiguous().float()
        cand_feat = cand_feat.contiguous().float()
        _check_shapes(cand_feat, self.n_cand, query_feat.shape[1], query_feat, self.pos_ptr)
        q = torch.as_tensor(np.asarray(queries, dtype=np.int32)).to(self.device)
        nq = int(q.numel())
        auc = torch.zeros(max(nq, 1), dtype=torch.float64, device=self.device)
        ap = torch.zeros_like(auc)
        flag = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.device)
        if nq:
            if int(q.min()) < 0 or int(q.max()) >= query_feat.shape[0]:
                raise IndexError("query index out of range")
            d = int(query_feat.shape[1])
            qb = int(max(16, min(nq, self.max_score_bytes // (4 * max(self.n_cand, 1)))))
            ws = self._grow(self._nbytes("dcue_rank_workspace_bytes", self.n_cand, d, qb))
            nat.check(nat.lib().dcue_rank_metrics(
                nat.ptr(query_feat), query_feat.shape[0], nat.ptr(cand_feat), self.n_cand, d, nat.ptr(q), nq,
                nat.ptr(self.pos_ptr), nat.ptr(self.pos_idx), nat.ptr(self.cand_class), int(mode), qb,
                nat.ptr(ws), ws.numel(), nat.ptr(auc), nat.ptr(ap), nat.ptr(flag), nat.stream_handle(self.device)),
                "dcue_rank_metrics")
        auc, ap, flag = auc[:nq].cpu().numpy(), ap[:nq].cpu().numpy(), flag[:nq].cpu().numpy()
        ok = (flag & 1).astype(bool)
        nonfinite = (flag & 2).astype(bool)
        checked = nonfinite[:int(np.argmin(ok))] if (mode == nat.RANK_SPLIT and not ok.all()) else nonfinite
        if checked.any():
            raise _nonfinite_error(queries, checked)
        sane = ~nonfinite
        if not (np.all((auc[sane] >= 0.0) & (auc[sane] <= 1.0)) and np.all((ap[sane] >= 0.0) & (ap[sane] <= 1.0))):
            raise RuntimeError("dcue_rank_metrics: AUC / AP outside [0, 1]")
        return auc, ap, ok


def identity_csr(n):
    """Each row excludes itself (DCUE.similar_songs: a song is not its own neighbour)."""
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)


class TopK(_Workspace):
    """Device-resident exclusion lists and candidate mask of one recommendation setting and the
    grow-only workspace of dcue_topk -- RankEvaluator's counterpart for "the k best candidates".

    excl_ptr [n_query_rows + 1] int64 / excl_idx int32: per query row, the sorted candidates never to
    return (both None: no exclusion); cand_mask [n_cand] uint8 (None: every candidate; then n_cand
    must be given). score: "cosine" (nn.CosineSimilarity, dcue_topk) or "dot" (the inner product of the
    raw rows, dcue_topk_scored: what WRMF factors are ranked by)."""

    DEFAULT_QUERY_BATCH = 4096
    _div = None  # the Diversify of diversity= calls, made at the first one
    _gcap = None  # the GroupCap of max_per_group= calls, likewise
    _groups = None  # (the caller's group_of, its device copy, n_groups) of the last max_per_group= call
    _excl_np = None  # the exclusion CSR's host copy, for deepening rounds
    _prior = None  # (the caller's prior, its device copy) of the last prior= call
    cap_rounds_used = 0  # ranking rounds of the last max_per_group= call (1: no list was deepened)

    def __init__(self, excl_ptr, excl_idx, cand_mask, device, n_cand=None, score="cosine"):
        self.device = torch.device(device)
        self.score = _score_mode(score)
        if (excl_ptr is None) != (excl_idx is None):
            raise ValueError("excl_ptr and excl_idx go together")
        self.excl_ptr = self.excl_idx = None
        if excl_ptr is not None:
            self.excl_ptr, self.excl_idx = _upload_csr(excl_ptr, excl_idx, self.device)
        self.cand_mask, self.n_cand = _upload_mask(cand_mask, n_cand, self.device)

    def workspace_bytes(self, d, qb, k, cand_split=0):
        return self._nbytes("dcue_topk_workspace_bytes", self.n_cand, d, qb, k, cand_split)

    def _nonfinite(self, queries, bad):
        return (_nonfinite_error if self.score == nat.SCORE_COSINE else _nonfinite_dot_error)(queries, bad)

    def _prior_arg(self, prior):
        """The float32 [n_cand] device copy of a prior= array or tensor (None stays None); the upload is kept
        for the next call with the same object. Finiteness is checked once, on the host array, before it."""
        if prior is None:
            return None
        if self._prior is None or self._prior[0] is not prior:
            host = prior.detach().cpu().numpy() if torch.is_tensor(prior) else np.asarray(prior)
            host = np.ascontiguousarray(host, dtype=np.float32).reshape(-1)
            if host.size != self.n_cand:
                raise ValueError("prior has %d entries for %d candidates" % (host.size, self.n_cand))
            if not np.isfinite(host).all():
                raise ValueError("prior is not finite at candidate %d" % int(np.argmin(np.isfinite(host))))
            self._prior = (prior, torch.from_numpy(host).to(self.device))
        return self._prior[1]

    def _diverse_raw(self, query_feat, cand_feat, queries, k, query_batch, cand_split, diversity, pool, rel,
                     groups=None, prior=None):
        """topk_raw at k = pool, then Diversify.mmr_raw down to k. The flags are dcue_topk's; a list MMR
        found non-finite (nat.LIST_FLAG_NONFINITE) carries dcue_topk's bit for it. groups (_group_args): the
        pool is capped per group before MMR sees it."""
        k, pool = check_pool(k, pool)
        if rel is None:  # (with a prior the sum is no longer on the similarity's scale)
            rel = "raw" if self.score == nat.SCORE_COSINE and prior is None else "minmax"
        if self._div is None:
            self._div = Diversify(self.device)
        idx, score, count, flags = self.topk_raw(query_feat, cand_feat, queries, pool, query_batch, cand_split,
                                                 prior=prior)
        gflags = None
        if groups is not None:  # MMR picks from a pool that already satisfies the cap, so its output does too
            idx, score, count, _, gflags = self._cap().cap_raw(idx, score, count, *groups, pool)
        idx, score, count, mflags = self._div.mmr_raw(idx, score, count, cand_feat, k, diversity, rel)
        flags = flags | ((mflags & nat.LIST_FLAG_NONFINITE) >> 1)
        if gflags is not None:
            flags = flags | (gflags & nat.GROUP_FLAG_BAD_GROUP) | (count < k).int() * nat.GROUP_FLAG_SHORT
        return idx, score, count, flags

    def _cap(self):
        if self._gcap is None:
            self._gcap = GroupCap(self.device)
        return self._gcap

    def _group_args(self, group_of, max_per_group, cap_rounds):
        """(group_of int32 [n_cand] on the device, n_groups, cap) of a max_per_group= call; the uploaded
        map is kept for the next call with the same array."""
        if group_of is None:
            raise ValueError("max_per_group needs group_of, the candidates' groups")
        cap, cap_rounds = int(max_per_group), int(cap_rounds)
        if cap < 1:
            raise ValueError("max_per_group must be at least 1, got %d" % cap)
        if cap_rounds < 1:
            raise ValueError("cap_rounds must be at least 1, got %d" % cap_rounds)
        if self._groups is None or self._groups[0] is not group_of:
            g = group_of if torch.is_tensor(group_of) else torch.from_numpy(np.ascontiguousarray(group_of, np.int32))
            g = g.to(self.device, torch.int32).contiguous().reshape(-1)
            if g.numel() != self.n_cand:
                raise ValueError("group_of has %d entries for %d candidates" % (g.numel(), self.n_cand))
            self._groups = (group_of, g, max(int(g.max()) + 1, 0))
        return self._groups[1], self._groups[2], cap

    def _excl_host(self):
        """The base exclusion CSR as numpy arrays (None, None without one), copied back once."""
        if self._excl_np is None and self.excl_ptr is not None:
            self._excl_np = (self.excl_ptr.cpu().numpy(), self.excl_idx.cpu().numpy())
        return self._excl_np if self._excl_np is not None else (None, None)

    def _capped_raw(self, query_feat, cand_feat, queries, k, query_batch, cand_split, pool, groups, cap_rounds,
                    prior=None):
        """topk_raw at k = pool, GroupCap.cap_raw down to k, and up to cap_rounds - 1 deepening rounds for
        the lists the cap left short of k while their pool was full: those lists' query rows are ranked
        again at k = pool with everything ranked so far added to their exclusion rows -- a score is a
        function of the two rows and d alone, so this is the next `pool` entries of the same total order
        -- and the cap continues with the entries kept so far as its carry. A list that comes back
        without GROUP_FLAG_SHORT equals the cap applied to the full ranking. The deepening CSR is built
        on the host (the rare path)."""
        k, pool = check_pool(k, pool)
        queries = np.asarray(queries, dtype=np.int64).reshape(-1)
        idx, score, count, flags = self.topk_raw(query_feat, cand_feat, queries, pool, query_batch, cand_split,
                                                 prior=prior)
        gc = self._cap()
        oidx, oscore, ocount, _, gflags = gc.cap_raw(idx, score, count, *groups, k)
        self.cap_rounds_used = 1
        ranked = {}  # list -> every pool entry ranked for it so far
        for _ in range(int(cap_rounds) - 1):
            rows = torch.nonzero(((gflags & nat.GROUP_FLAG_SHORT) != 0) & (count == pool)).reshape(-1)
            if rows.numel() == 0:
                break
            self.cap_rounds_used += 1
            rows_np = rows.cpu().numpy()
            for r, entries in zip(rows_np, idx.index_select(0, rows).cpu().numpy()):
                ranked[r] = np.concatenate([ranked[r], entries]) if r in ranked else entries
            bptr, bidx = self._excl_host()
            excl = [np.union1d(ranked[r], bidx[bptr[queries[r]]:bptr[queries[r] + 1]]) if bptr is not None
                    else np.unique(ranked[r]) for r in rows_np]
            qrows = torch.as_tensor(queries[rows_np]).to(self.device)
            deeper = TopK(*histories_csr(excl), self.cand_mask, self.device, n_cand=self.n_cand,
                          score=[s for s, v in nat.SCORES.items() if v == self.score][0])
            didx, dscore, dcount, dflags = deeper.topk_raw(query_feat.index_select(0, qrows), cand_feat,
                                                           np.arange(len(rows_np)), pool, query_batch, cand_split,
                                                           prior=prior)
            carry = (oidx.index_select(0, rows), oscore.index_select(0, rows), ocount.index_select(0, rows))
            nidx, nscore, ncount, _, nflags = gc.cap_raw(didx, dscore, dcount, *groups, k, carry=carry)
            idx[rows], count[rows] = didx, dcount  # the pools the next round continues from
            oidx[rows], oscore[rows], ocount[rows], gflags[rows] = nidx, nscore, ncount, nflags
            flags[rows] |= dflags
        return oidx, oscore, ocount, flags | (gflags & (nat.GROUP_FLAG_SHORT | nat.GROUP_FLAG_BAD_GROUP))

    def topk_raw(self, query_feat, cand_feat, queries, k, query_batch=None, cand_split=0, diversity=None, pool=None,
                 rel=None, group_of=None, max_per_group=None, cap_rounds=4, prior=None):
        """(idx int32 [n, k], score float32 [n, k], count int32 [n], flags int32 [n]) device tensors,
        as dcue_topk writes them (no non-finite check).

        diversity (lambda in [0, 1]; None: the plain relevance ranking, today's path exactly): the
        `pool` best candidates are ranked (default min(128, 4 k); k <= pool <= 128) and re-ranked down
        to k by Maximal Marginal Relevance on the device (Diversify.mmr_raw, include/dcue.h
        dcue_list_mmr). rel: "raw" / "minmax" relevance scaling, default raw for cosine scores and
        minmax for dot. The scores returned are the entries' original ones.

        max_per_group (None: no cap, today's path exactly) with group_of, an int array [n_cand] of each
        candidate's group (artist, album, ...; -1: ungrouped, never capped): no group holds more than
        max_per_group entries of a list (GroupCap.cap_raw, include/dcue.h dcue_list_group_cap). The
        `pool` best candidates are ranked and capped down to k; lists the cap leaves short while their
        pool was full are deepened, at most cap_rounds - 1 times (_capped_raw). flags then also carries
        nat.GROUP_FLAG_SHORT (fewer than k entries: the catalogue or the rounds ran out) and
        GROUP_FLAG_BAD_GROUP. With diversity= the pool is capped first and MMR picks from the capped pool,
        without deepening.

        prior (None: today's path exactly): a float array or tensor [n_cand] added to every score of its
        candidate inside the fused ranking (include/dcue.h dcue_topk_prior): s = fl32(s0 + prior[c]), and
        the scores returned are the sums. It reaches every ranking the call makes -- the pool of
        diversity=, the first round and the deepening rounds of max_per_group= -- and with it rel defaults
        to "minmax" in both score modes. A non-finite entry raises ValueError before anything is uploaded."""
        prior_dev = self._prior_arg(prior)
        if max_per_group is not None:
            groups = self._group_args(group_of, max_per_group, cap_rounds)
            if diversity is not None:
                return self._diverse_raw(query_feat, cand_feat, queries, k, query_batch, cand_split, diversity, pool,
                                         rel, groups, prior)
            if rel is not None:
                raise ValueError("rel belongs to diversity=, which is not set")
            return self._capped_raw(query_feat, cand_feat, queries, k, query_batch, cand_split, pool, groups,
                                    cap_rounds, prior)
        if group_of is not None:
            raise ValueError("group_of belongs to max_per_group=, which is not set")
        if diversity is not None:
            return self._diverse_raw(query_feat, cand_feat, queries, k, query_batch, cand_split, diversity, pool, rel,
                                     prior=prior)
        if pool is not None or rel is not None:
            raise ValueError("pool and rel belong to diversity= (pool also to max_per_group=), which is not set")
        nat.require_gpu(query_feat, "query_feat")
        nat.require_gpu(cand_feat, "cand_feat")
        query_feat = query_feat.contiguous().float()
        cand_feat = cand_feat.contiguous().float()
        _check_shapes(cand_feat, self.n_cand, query_feat.shape[1], query_feat, self.excl_ptr)
        k = int(k)
        if not 1 <= k <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, k))
        q = torch.as_tensor(np.asarray(queries, dtype=np.int32)).to(self.device)
        nq = int(q.numel())
        idx = torch.full((max(nq, 1), k), -1, dtype=torch.int32, device=self.device)
        score = torch.full((max(nq, 1), k), float("-inf"), dtype=torch.float32, device=self.device)
        count = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.device)
        flags = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.device)
        if nq:
            if int(q.min()) < 0 or int(q.max()) >= query_feat.shape[0]:
                raise IndexError("query index out of range")
            d = int(query_feat.shape[1])
            qb = int(min(nq, self.DEFAULT_QUERY_BATCH if query_batch is None else query_batch))
            ws = self._grow(self.workspace_bytes(d, qb, k, int(cand_split)))
            args = (nat.ptr(query_feat), query_feat.shape[0], nat.ptr(cand_feat), self.n_cand, d, nat.ptr(q), nq,
                    nat.ptr(self.excl_ptr), nat.ptr(self.excl_idx), nat.ptr(self.cand_mask), k, qb, int(cand_split),
                    nat.ptr(ws), ws.numel(), nat.ptr(idx), nat.ptr(score), nat.ptr(count), nat.ptr(flags),
                    nat.stream_handle(self.device))
            if prior_dev is not None:
                nat.check(nat.lib().dcue_topk_prior(self.score, *args[:10], nat.ptr(prior_dev), *args[10:]),
                          "dcue_topk_prior")
            elif self.score == nat.SCORE_COSINE:
                nat.check(nat.lib().dcue_topk(*args), "dcue_topk")
            else:
                nat.check(nat.lib().dcue_topk_scored(self.score, *args), "dcue_topk_scored")
        return idx[:nq], score[:nq], count[:nq], flags[:nq]

    def topk(self, query_feat, cand_feat, queries, k, query_batch=None, cand_split=0, diversity=None, pool=None,
             rel=None, group_of=None, max_per_group=None, cap_rounds=4, prior=None):
        """(idx int64 [n, k], score float32 [n, k], count int32 [n]) numpy arrays, best first; rows
        with fewer than k eligible candidates end in idx -1 / score -inf. diversity / pool / rel: as
        topk_raw (the lists are then in MMR's selection order, not sorted by score). group_of /
        max_per_group / cap_rounds: as topk_raw; a group id outside -1 .. n_groups - 1 raises ValueError.
        prior: as topk_raw (the scores are then the sums).

        Raises ValueError in the evaluator's wording when an eligible candidate's score is NaN or
        infinite: a diverged model fails here as it fails in DCUE.score (score="dot": the factors are
        not finite or the product overflowed)."""
        idx, score, count, flags = self.topk_raw(query_feat, cand_feat, queries, k, query_batch, cand_split,
                                                 diversity, pool, rel, group_of, max_per_group, cap_rounds, prior)
        flags = flags.cpu().numpy()
        bad = (flags & 2).astype(bool)
        if bad.any():
            raise self._nonfinite(queries, bad)
        if (flags & nat.GROUP_FLAG_BAD_GROUP).any():
            raise ValueError("group_of holds a group id below -1")
        return idx.cpu().numpy().astype(np.int64), score.cpu().numpy(), count.cpu().numpy()


def check_cutoffs(ks):
    """The sorted distinct cutoffs of `ks` as a list of ints; ValueError naming the limit otherwise."""
    ks = sorted({int(k) for k in ks})
    if not ks:
        raise ValueError("ks is empty: at least 1 cutoff is needed")
    if len(ks) > nat.TOPK_METRICS_MAX_CUTOFFS:
        raise ValueError("at most %d cutoffs per call, got %d" % (nat.TOPK_METRICS_MAX_CUTOFFS, len(ks)))
    if ks[0] < 1 or ks[-1] > nat.TOPK_MAX_K:
        raise ValueError("cutoffs must be in 1..%d, got %s" % (nat.TOPK_MAX_K, ks))
    return ks


def check_pool(k, pool):
    """(k, pool) as ints for a diversity= call: pool defaults to min(128, 4 k); ValueError naming the
    limits otherwise."""
    k = int(k)
    if not 1 <= k <= nat.TOPK_MAX_K:
        raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, k))
    pool = min(nat.TOPK_MAX_K, 4 * k) if pool is None else int(pool)
    if not k <= pool <= nat.TOPK_MAX_K:
        raise ValueError("pool must be in k..%d (k = %d), got %d" % (nat.TOPK_MAX_K, k, pool))
    return k, pool


class Diversify(_Workspace):
    """Maximal Marginal Relevance re-ranking and intra-list diversity of the lists dcue_topk leaves on
    the device (include/dcue.h dcue_list_mmr / dcue_list_ild / dcue_list_ild_mean): device tensors in
    and out, one kernel launch per call, no list is copied to the host."""

    def __init__(self, device):
        self.device = torch.device(device)

    def _device_lists(self, idx, count, cand_feat, score=None):
        nat.require_gpu(idx, "idx")
        nat.require_gpu(count, "count")
        nat.require_gpu(cand_feat, "cand_feat")
        if idx.dim() != 2 or idx.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() != idx.shape[0]:
            raise ValueError("idx must be int32 [n, k] and count int32 [n]")
        if not 1 <= idx.shape[1] <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, idx.shape[1]))
        if cand_feat.dim() != 2 or cand_feat.shape[0] < 1 or not 1 <= cand_feat.shape[1] <= 256:
            raise ValueError("candidate factors must be [n_cand, d] with d in 1..256, got %s"
                             % (tuple(cand_feat.shape),))
        if score is not None:
            nat.require_gpu(score, "score")
            if score.dtype != torch.float32 or score.shape != idx.shape:
                raise ValueError("score must be float32 %s like idx, got %s %s"
                                 % (tuple(idx.shape), score.dtype, tuple(score.shape)))
            score = score.contiguous()
        return idx.contiguous(), count.contiguous(), cand_feat.contiguous().float(), score

    def _workspace(self, pool, d, n):
        """(pointer, bytes) of the grown workspace; (None, 0) while the kernels need none."""
        nbytes = self._nbytes("dcue_list_mmr_workspace_bytes", pool, d, n)
        return (nat.ptr(self._grow(nbytes)), nbytes) if nbytes else (None, 0)

    def mmr_raw(self, idx, score, count, cand_feat, k, lambda_, rel="raw"):
        """(idx int32 [n, k], score float32 [n, k], count int32 [n], flags int32 [n]) device tensors: the
        pools idx int32 [n, pool] / score float32 [n, pool] / count int32 [n] (as dcue_topk writes them)
        re-ranked down to k by MMR with lambda = lambda_ over the cosine of cand_feat's rows. rel: "raw"
        or "minmax". score is each entry's original one; flags: nat.LIST_FLAG_BAD_INDEX /
        LIST_FLAG_NONFINITE (such a list comes back empty)."""
        idx, count, cand_feat, score = self._device_lists(idx, count, cand_feat, score)
        n, pool, k, lam = int(idx.shape[0]), int(idx.shape[1]), int(k), float(lambda_)
        if not 1 <= k <= pool:
            raise ValueError("k must be in 1..%d (the pool), got %d" % (pool, k))
        if not 0.0 <= lam <= 1.0:
            raise ValueError("lambda must be in [0, 1], got %r" % (lambda_,))
        if rel not in nat.MMR_RELS:
            raise ValueError("rel must be one of %s, got %r" % (sorted(nat.MMR_RELS), rel))
        out_idx = torch.full((max(n, 1), k), -1, dtype=torch.int32, device=self.device)
        out_score = torch.full((max(n, 1), k), float("-inf"), dtype=torch.float32, device=self.device)
        out_count = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        if n:
            d = int(cand_feat.shape[1])
            ws, ws_bytes = self._workspace(pool, d, n)
            nat.check(nat.lib().dcue_list_mmr(
                nat.ptr(idx), nat.ptr(score), nat.ptr(count), n, pool, nat.ptr(cand_feat), int(cand_feat.shape[0]), d,
                lam, nat.MMR_RELS[rel], k, ws, ws_bytes, nat.ptr(out_idx), nat.ptr(out_score), nat.ptr(out_count),
                nat.ptr(flags), nat.stream_handle(self.device)), "dcue_list_mmr")
        return out_idx[:n], out_score[:n], out_count[:n], flags[:n]

    def _ild_into(self, idx, count, cand_feat, ks, cut, out, flags):
        """dcue_list_ild on checked device lists, writing out [n, m] / flags [n] (views of the caller's buffers)."""
        n, k, d = int(idx.shape[0]), int(idx.shape[1]), int(cand_feat.shape[1])
        if ks[-1] > k:
            raise ValueError("cutoff %d is beyond the lists' k = %d" % (ks[-1], k))
        if n:
            ws, ws_bytes = self._workspace(k, d, n)
            nat.check(nat.lib().dcue_list_ild(
                nat.ptr(idx), nat.ptr(count), n, k, nat.ptr(cand_feat), int(cand_feat.shape[0]), d,
                ctypes.cast(cut, ctypes.c_void_p), len(ks), ws, ws_bytes, nat.ptr(out), nat.ptr(flags),
                nat.stream_handle(self.device)), "dcue_list_ild")

    def ild_raw(self, idx, count, cand_feat, ks):
        """(ild float64 [n, m], flags int32 [n]) device tensors: the intra-list diversity of the lists
        idx int32 [n, k] / count int32 [n] at the sorted distinct cutoffs of ks. flags:
        nat.LIST_FLAG_NO_PAIR (a cutoff with fewer than two entries: its value is 0) / LIST_FLAG_BAD_INDEX /
        LIST_FLAG_NONFINITE."""
        ks = check_cutoffs(ks)
        cut = (ctypes.c_int32 * len(ks))(*ks)
        idx, count, cand_feat, _ = self._device_lists(idx, count, cand_feat)
        n = int(idx.shape[0])
        out = torch.zeros((max(n, 1), len(ks)), dtype=torch.float64, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self._ild_into(idx, count, cand_feat, ks, cut, out, flags)
        return out[:n], flags[:n]

    def ild_mean_raw(self, ild, flags):
        """(mean float64 [m], n_evaluated int32 [1]) device tensors: dcue_list_ild_mean over ild [n, m] /
        flags [n] -- the mean over the unflagged lists, in an order that depends on n and m only."""
        nat.require_gpu(ild, "ild")
        nat.require_gpu(flags, "flags")
        if ild.dim() != 2 or ild.dtype != torch.float64 or flags.dtype != torch.int32 or flags.numel() != ild.shape[0]:
            raise ValueError("ild must be float64 [n, m] and flags int32 [n]")
        n, m = int(ild.shape[0]), int(ild.shape[1])
        if not 1 <= m <= nat.TOPK_METRICS_MAX_CUTOFFS:
            raise ValueError("at most %d cutoffs per call, got %d" % (nat.TOPK_METRICS_MAX_CUTOFFS, m))
        mean = torch.zeros(m, dtype=torch.float64, device=self.device)
        n_eval = torch.zeros(1, dtype=torch.int32, device=self.device)
        if n == 0:  # (an empty tensor's address may be null)
            ild = torch.zeros((1, m), dtype=torch.float64, device=self.device)
            flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_list_ild_mean(nat.ptr(ild.contiguous()), nat.ptr(flags.contiguous()), n, m,
                                               nat.ptr(mean), nat.ptr(n_eval), nat.stream_handle(self.device)),
                  "dcue_list_ild_mean")
        return mean, n_eval


def check_group_flags(queries, flags):
    """Raises for the first flagged list of a GroupCap call: IndexError for an index out of range
    (nat.LIST_FLAG_BAD_INDEX), ValueError for a group id outside -1 .. n_groups - 1
    (nat.GROUP_FLAG_BAD_GROUP). GROUP_FLAG_SHORT is no error. flags: the call's int32 [n] tensor or array."""
    flags = flags.cpu().numpy() if torch.is_tensor(flags) else np.asarray(flags)
    bad = (flags & nat.LIST_FLAG_BAD_INDEX).astype(bool)
    if bad.any():
        raise IndexError("list or carried index out of range (query %d)"
                         % int(np.asarray(queries).reshape(-1)[int(np.argmax(bad))]))
    bad = (flags & nat.GROUP_FLAG_BAD_GROUP).astype(bool)
    if bad.any():
        raise ValueError("group id outside -1 .. n_groups - 1 (query %d)"
                         % int(np.asarray(queries).reshape(-1)[int(np.argmax(bad))]))


class GroupCap(_Workspace):
    """Per-group caps and group statistics of the lists dcue_topk / dcue_list_mmr leave on the device
    (include/dcue.h dcue_list_group_cap / dcue_list_group_stats / dcue_list_group_stats_mean): device
    tensors in and out, one kernel launch per call, no list is copied to the host. A group is whatever
    group_of says -- artist, album, label; -1 is "ungrouped"."""

    def __init__(self, device):
        self.device = torch.device(device)

    def _lists(self, idx, count, group_of, n_groups, score=None):
        for t, name in ((idx, "idx"), (count, "count"), (group_of, "group_of")):
            nat.require_gpu(t, name)
        if idx.dim() != 2 or idx.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() != idx.shape[0]:
            raise ValueError("idx must be int32 [n, k] and count int32 [n]")
        if not 1 <= idx.shape[1] <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, idx.shape[1]))
        if group_of.dtype != torch.int32 or group_of.dim() != 1 or group_of.numel() < 1:
            raise ValueError("group_of must be int32 [n_cand]")
        if not 0 <= int(n_groups) <= 2 ** 31 - 1:
            raise ValueError("n_groups must be in 0..2^31 - 1, got %d" % n_groups)
        if score is not None:
            nat.require_gpu(score, "score")
            if score.dtype != torch.float32 or score.shape != idx.shape:
                raise ValueError("score must be float32 %s like idx, got %s %s"
                                 % (tuple(idx.shape), score.dtype, tuple(score.shape)))
            score = score.contiguous()
        return idx.contiguous(), count.contiguous(), group_of.contiguous(), score

    def cap_raw(self, idx, score, count, group_of, n_groups, cap, k_out, carry=None):
        """(idx int32 [n, k_out], score float32 [n, k_out], count int32 [n], dropped int32 [n], flags int32
        [n]) device tensors: the pools idx int32 [n, pool] / score float32 [n, pool] / count int32 [n] (as
        dcue_topk writes them) cut down to at most `cap` entries per group of group_of (int32 [n_cand] on
        the device), in pool order, k_out at the most. carry: (idx [n, k_out], score [n, k_out], count [n])
        of entries an earlier call kept -- they come first, unchanged, and count toward their groups.
        dropped: the pool positions the cap removed before the list filled. flags:
        nat.LIST_FLAG_BAD_INDEX / GROUP_FLAG_BAD_GROUP (such a list comes back empty) and GROUP_FLAG_SHORT
        (fewer than k_out entries; they are valid)."""
        idx, count, group_of, score = self._lists(idx, count, group_of, n_groups, score)
        n, pool, k_out, cap = int(idx.shape[0]), int(idx.shape[1]), int(k_out), int(cap)
        if score is None:
            raise ValueError("score is needed")
        if cap < 1:
            raise ValueError("cap must be at least 1, got %d" % cap)
        if not 1 <= k_out <= nat.TOPK_MAX_K:
            raise ValueError("k_out must be in 1..%d, got %d" % (nat.TOPK_MAX_K, k_out))
        cidx = cscore = ccount = None
        if carry is not None:
            cidx, cscore, ccount = carry
            for t, name in ((cidx, "carry idx"), (cscore, "carry score"), (ccount, "carry count")):
                nat.require_gpu(t, name)
            if (cidx.dtype != torch.int32 or cscore.dtype != torch.float32 or ccount.dtype != torch.int32
                    or tuple(cidx.shape) != (n, k_out) or tuple(cscore.shape) != (n, k_out) or ccount.numel() != n):
                raise ValueError("carry must be (int32 [n, k_out], float32 [n, k_out], int32 [n])")
            cidx, cscore, ccount = cidx.contiguous(), cscore.contiguous(), ccount.contiguous()
        out_idx = torch.full((max(n, 1), k_out), -1, dtype=torch.int32, device=self.device)
        out_score = torch.full((max(n, 1), k_out), float("-inf"), dtype=torch.float32, device=self.device)
        out_count = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        dropped = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        if n:
            nat.check(nat.lib().dcue_list_group_cap(
                nat.ptr(idx), nat.ptr(score), nat.ptr(count), n, pool, nat.ptr(group_of), int(group_of.numel()),
                int(n_groups), cap, k_out, nat.ptr(cidx), nat.ptr(cscore), nat.ptr(ccount), nat.ptr(out_idx),
                nat.ptr(out_score), nat.ptr(out_count), nat.ptr(dropped), nat.ptr(flags),
                nat.stream_handle(self.device)), "dcue_list_group_cap")
        return out_idx[:n], out_score[:n], out_count[:n], dropped[:n], flags[:n]

    def _stats_into(self, idx, count, group_of, n_groups, ks, cut, out, flags, exposure):
        """dcue_list_group_stats on checked device lists, writing out [n, m, 2] / flags [n] (views of the
        caller's buffers) and accumulating into exposure (or None)."""
        n, k = int(idx.shape[0]), int(idx.shape[1])
        if ks[-1] > k:
            raise ValueError("cutoff %d is beyond the lists' k = %d" % (ks[-1], k))
        if exposure is not None and (exposure.dtype != torch.int32 or tuple(exposure.shape) != (len(ks), n_groups)):
            raise ValueError("exposure must be int32 [%d, %d]" % (len(ks), n_groups))
        if n:
            nat.check(nat.lib().dcue_list_group_stats(
                nat.ptr(idx), nat.ptr(count), n, k, nat.ptr(group_of), int(group_of.numel()), int(n_groups),
                ctypes.cast(cut, ctypes.c_void_p), len(ks), nat.ptr(out), nat.ptr(flags), nat.ptr(exposure),
                nat.stream_handle(self.device)), "dcue_list_group_stats")

    def stats_raw(self, idx, count, group_of, n_groups, ks, exposure=None):
        """(stats int32 [n, m, 2], flags int32 [n]) device tensors for the lists idx int32 [n, k] / count
        int32 [n] at the sorted distinct cutoffs of ks: per cutoff K the number of distinct groups among
        the first min(K, count) entries (each ungrouped entry one of its own) and the most entries one
        group holds. exposure: an int32 [m, n_groups] device tensor to accumulate into (new_exposure), or
        None. A flagged list (LIST_FLAG_BAD_INDEX / GROUP_FLAG_BAD_GROUP) has zeros and adds no exposure."""
        ks = check_cutoffs(ks)
        cut = (ctypes.c_int32 * len(ks))(*ks)
        idx, count, group_of, _ = self._lists(idx, count, group_of, n_groups)
        n = int(idx.shape[0])
        out = torch.zeros((max(n, 1), len(ks), nat.GROUP_N_STATS), dtype=torch.int32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self._stats_into(idx, count, group_of, int(n_groups), ks, cut, out, flags, exposure)
        return out[:n], flags[:n]

    def new_exposure(self, m, n_groups):
        return torch.zeros((m, max(int(n_groups), 1)), dtype=torch.int32, device=self.device)[:, :int(n_groups)]

    def mean_raw(self, stats, flags, exposure=None, present=None):
        """(mean float64 [m, 2], coverage float64 [m] or None, n_evaluated int32 [1]) device tensors:
        dcue_list_group_stats_mean over stats [n, m, 2] / flags [n] -- exact int64 sums over the unflagged
        lists and one division each. exposure (int32 [m, n_groups], contiguous): adds the share of groups
        exposed up to each cutoff among those with a non-zero byte in present (uint8 [n_groups] on the
        device; None: all groups)."""
        nat.require_gpu(stats, "stats")
        nat.require_gpu(flags, "flags")
        if (stats.dim() != 3 or stats.shape[2] != nat.GROUP_N_STATS or stats.dtype != torch.int32
                or flags.dtype != torch.int32 or flags.numel() != stats.shape[0]):
            raise ValueError("stats must be int32 [n, m, 2] and flags int32 [n]")
        n, m = int(stats.shape[0]), int(stats.shape[1])
        if not 1 <= m <= nat.TOPK_METRICS_MAX_CUTOFFS:
            raise ValueError("at most %d cutoffs per call, got %d" % (nat.TOPK_METRICS_MAX_CUTOFFS, m))
        n_groups = 0
        if exposure is not None:
            if exposure.dtype != torch.int32 or exposure.dim() != 2 or exposure.shape[0] != m:
                raise ValueError("exposure must be int32 [%d, n_groups]" % m)
            n_groups = int(exposure.shape[1])
            exposure = exposure.contiguous() if n_groups else torch.zeros((m, 1), dtype=torch.int32, device=self.device)
            if present is not None and (present.dtype != torch.uint8 or present.numel() != n_groups):
                raise ValueError("present must be uint8 [%d]" % n_groups)
        mean = torch.zeros((m, nat.GROUP_N_STATS), dtype=torch.float64, device=self.device)
        cov = torch.zeros(m, dtype=torch.float64, device=self.device) if exposure is not None else None
        n_eval = torch.zeros(1, dtype=torch.int32, device=self.device)
        if n == 0:  # (an empty tensor's address may be null)
            stats = torch.zeros((1, m, nat.GROUP_N_STATS), dtype=torch.int32, device=self.device)
            flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_list_group_stats_mean(
            nat.ptr(stats.contiguous()), nat.ptr(flags.contiguous()), n, m, nat.ptr(exposure),
            nat.ptr(present.contiguous() if present is not None and n_groups else None), n_groups, nat.ptr(mean),
            nat.ptr(cov), nat.ptr(n_eval), nat.stream_handle(self.device)), "dcue_list_group_stats_mean")
        return mean, cov, n_eval


class PopStats(_Workspace):
    """Popularity-bias statistics of the lists dcue_topk / dcue_list_mmr / dcue_list_group_cap leave on the
    device (include/dcue.h dcue_list_item_stats / dcue_list_item_stats_mean / dcue_exposure_gini): device
    tensors in and out, no list is copied to the host.

    item_value float64 [n_cand] (None: the column is 0): a per-item number prepared on the host -- the
    self-information of DCUE.set_popularity gives novelty; item_tail uint8 [n_cand] (None: 0): non-zero
    for a long-tail item."""

    def __init__(self, device, n_cand, item_value=None, item_tail=None):
        self.device = torch.device(device)
        self.n_cand = int(n_cand)
        self.item_value = self._column(item_value, torch.float64, np.float64, "item_value")
        self.item_tail = self._column(item_tail, torch.uint8, np.uint8, "item_tail")

    def _column(self, a, tdtype, ndtype, name):
        if a is None:
            return None
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=ndtype))
        t = t.to(self.device, tdtype).contiguous().reshape(-1)
        if t.numel() != self.n_cand:
            raise ValueError("%s has %d entries for %d candidates" % (name, t.numel(), self.n_cand))
        return t

    def _stats_into(self, idx, count, ks, cut, out, flags):
        """dcue_list_item_stats on checked device lists, writing out [n, m, 2] / flags [n] (views of the
        caller's buffers)."""
        n, k = int(idx.shape[0]), int(idx.shape[1])
        if ks[-1] > k:
            raise ValueError("cutoff %d is beyond the lists' k = %d" % (ks[-1], k))
        if n:
            nat.check(nat.lib().dcue_list_item_stats(
                nat.ptr(idx), nat.ptr(count), n, k, nat.ptr(self.item_value), nat.ptr(self.item_tail), self.n_cand,
                ctypes.cast(cut, ctypes.c_void_p), len(ks), nat.ptr(out), nat.ptr(flags),
                nat.stream_handle(self.device)), "dcue_list_item_stats")

    def stats_raw(self, idx, count, ks):
        """(stats float64 [n, m, 2], flags int32 [n]) device tensors for the lists idx int32 [n, k] / count
        int32 [n] at the sorted distinct cutoffs of ks: per cutoff K the mean item_value and the share of
        tail items among the first min(K, count) entries. flags: nat.ITEM_FLAG_EMPTY / LIST_FLAG_BAD_INDEX
        (such a list has zeros and is left out of the means)."""
        ks = check_cutoffs(ks)
        cut = (ctypes.c_int32 * len(ks))(*ks)
        nat.require_gpu(idx, "idx")
        nat.require_gpu(count, "count")
        if idx.dim() != 2 or idx.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() != idx.shape[0]:
            raise ValueError("idx must be int32 [n, k] and count int32 [n]")
        if not 1 <= idx.shape[1] <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, idx.shape[1]))
        n = int(idx.shape[0])
        out = torch.zeros((max(n, 1), len(ks), nat.ITEM_N_STATS), dtype=torch.float64, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self._stats_into(idx.contiguous(), count.contiguous(), ks, cut, out, flags)
        return out[:n], flags[:n]

    def mean_raw(self, stats, flags):
        """(mean float64 [m, 2], n_evaluated int32 [1]) device tensors: dcue_list_item_stats_mean over stats
        [n, m, 2] / flags [n] -- the mean over the unflagged lists, in an order that depends on n and m only."""
        nat.require_gpu(stats, "stats")
        nat.require_gpu(flags, "flags")
        if (stats.dim() != 3 or stats.shape[2] != nat.ITEM_N_STATS or stats.dtype != torch.float64
                or flags.dtype != torch.int32 or flags.numel() != stats.shape[0]):
            raise ValueError("stats must be float64 [n, m, 2] and flags int32 [n]")
        n, m = int(stats.shape[0]), int(stats.shape[1])
        if not 1 <= m <= nat.TOPK_METRICS_MAX_CUTOFFS:
            raise ValueError("at most %d cutoffs per call, got %d" % (nat.TOPK_METRICS_MAX_CUTOFFS, m))
        mean = torch.zeros((m, nat.ITEM_N_STATS), dtype=torch.float64, device=self.device)
        n_eval = torch.zeros(1, dtype=torch.int32, device=self.device)
        if n == 0:  # (an empty tensor's address may be null)
            stats = torch.zeros((1, m, nat.ITEM_N_STATS), dtype=torch.float64, device=self.device)
            flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_list_item_stats_mean(nat.ptr(stats.contiguous()), nat.ptr(flags.contiguous()), n, m,
                                                      nat.ptr(mean), nat.ptr(n_eval), nat.stream_handle(self.device)),
                  "dcue_list_item_stats_mean")
        return mean, n_eval

    def gini_raw(self, exposure, n_lists_max, cand_mask=None):
        """(gini float64 [m], total int64 [m]) device tensors: the Gini index of the exposure counts
        (int32 [m, n_cand] on the device, as dcue_topk_metrics accumulates them; cutoff i counts the
        positions below it, as coverage does) over the candidates cand_mask (uint8 [n_cand] on the device;
        None: all) admits, and the exposure they sum to. n_lists_max: the lists that added to `exposure`;
        a count above it gives total -1 (gini raises for it)."""
        nat.require_gpu(exposure, "exposure")
        if exposure.dim() != 2 or exposure.dtype != torch.int32 or exposure.shape[1] != self.n_cand:
            raise ValueError("exposure must be int32 [m, %d]" % self.n_cand)
        m = int(exposure.shape[0])
        if not 1 <= m <= nat.TOPK_METRICS_MAX_CUTOFFS:
            raise ValueError("at most %d cutoffs per call, got %d" % (nat.TOPK_METRICS_MAX_CUTOFFS, m))
        if cand_mask is not None and (cand_mask.dtype != torch.uint8 or cand_mask.numel() != self.n_cand):
            raise ValueError("cand_mask must be uint8 [%d]" % self.n_cand)
        nbytes = self._nbytes("dcue_exposure_gini_workspace_bytes", self.n_cand, m, int(n_lists_max))
        ws = self._grow(nbytes)
        gini = torch.zeros(m, dtype=torch.float64, device=self.device)
        total = torch.zeros(m, dtype=torch.int64, device=self.device)
        nat.check(nat.lib().dcue_exposure_gini(
            nat.ptr(exposure.contiguous()), nat.ptr(cand_mask.contiguous() if cand_mask is not None else None),
            self.n_cand, m, nat.ptr(ws), nbytes, nat.ptr(gini), nat.ptr(total), nat.stream_handle(self.device)),
            "dcue_exposure_gini")
        return gini, total

    def gini(self, exposure, n_lists_max, cand_mask=None):
        """gini_raw's index as a float64 numpy array; ValueError where a count lies outside 0..n_lists_max."""
        g, total = self.gini_raw(exposure, n_lists_max, cand_mask)
        if (total.cpu().numpy() < 0).any():
            raise ValueError("an exposure count is negative or above n_lists_max = %d" % int(n_lists_max))
        return g.cpu().numpy()


def check_reasons(reasons):
    """`reasons` as an int in 1..EXPLAIN_MAX_REASONS; ValueError naming the limit otherwise."""
    m = int(reasons)
    if not 1 <= m <= nat.EXPLAIN_MAX_REASONS:
        raise ValueError("reasons must be in 1..%d, got %d" % (nat.EXPLAIN_MAX_REASONS, m))
    return m


def check_explain_flags(queries, flags):
    """Raises for the first flagged list of an explain call: IndexError for an index out of range
    (nat.LIST_FLAG_BAD_INDEX), ValueError in the evaluator's wording for a NaN or infinite similarity
    (nat.LIST_FLAG_NONFINITE). flags: the call's int32 [n] tensor or array."""
    flags = flags.cpu().numpy() if torch.is_tensor(flags) else np.asarray(flags)
    bad = (flags & nat.LIST_FLAG_BAD_INDEX).astype(bool)
    if bad.any():
        raise IndexError("list, history or query index out of range (query %d)"
                         % int(np.asarray(queries).reshape(-1)[int(np.argmax(bad))]))
    bad = (flags & nat.LIST_FLAG_NONFINITE).astype(bool)
    if bad.any():
        raise _nonfinite_error(queries, bad)


class Explain(_Workspace):
    """"Because you played X" for the lists dcue_topk / dcue_list_mmr leave on the device (include/dcue.h
    dcue_list_explain): per pick, the songs of the query row's history with the largest cosine to it --
    the very score TopK reports for the pair -- in one kernel launch, no list copied to the host."""

    def __init__(self, device):
        self.device = torch.device(device)

    def explain_raw(self, idx, count, queries, hist_ptr, hist_idx, cand_feat, m, hist_mask=None):
        """(why_idx int32 [n, k, m], why_sim float32 [n, k, m], flags int32 [n]) device tensors for the
        lists idx int32 [n, k] / count int32 [n] (as dcue_topk writes them) of the query rows `queries`.
        hist_ptr / hist_idx: a CSR over query rows in dcue_topk's exclusion format (arrays, or tensors
        already on the device); hist_mask [n_cand] uint8 (None: every entry counts): 0 keeps a song out
        of every history. Short rows end in -1 / -inf. flags: nat.EXPLAIN_FLAG_NO_HISTORY /
        LIST_FLAG_BAD_INDEX (the list is all padding) / LIST_FLAG_NONFINITE (no check is made here:
        check_explain_flags raises for them)."""
        m = check_reasons(m)
        nat.require_gpu(idx, "idx")
        nat.require_gpu(count, "count")
        nat.require_gpu(cand_feat, "cand_feat")
        if idx.dim() != 2 or idx.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() != idx.shape[0]:
            raise ValueError("idx must be int32 [n, k] and count int32 [n]")
        if not 1 <= idx.shape[1] <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, idx.shape[1]))
        if cand_feat.dim() != 2 or cand_feat.shape[0] < 1 or not 1 <= cand_feat.shape[1] <= 256:
            raise ValueError("candidate factors must be [n_cand, d] with d in 1..256, got %s"
                             % (tuple(cand_feat.shape),))
        idx, count, cand_feat = idx.contiguous(), count.contiguous(), cand_feat.contiguous().float()
        if torch.is_tensor(queries):
            q = queries.to(self.device, torch.int32).contiguous().reshape(-1)
        else:
            q = torch.as_tensor(np.asarray(queries, dtype=np.int32).reshape(-1)).to(self.device)
        n, k, n_cand, d = int(idx.shape[0]), int(idx.shape[1]), int(cand_feat.shape[0]), int(cand_feat.shape[1])
        if q.numel() != n:
            raise ValueError("%d queries for %d lists" % (q.numel(), n))
        n_rows = int(hist_ptr.numel() if torch.is_tensor(hist_ptr) else len(hist_ptr)) - 1
        if n_rows < 1:
            raise ValueError("the history CSR has no row")
        ptr, hidx = _upload_csr(hist_ptr, hist_idx, self.device)
        mask = None
        if hist_mask is not None:
            mask = (hist_mask if torch.is_tensor(hist_mask)
                    else torch.from_numpy(np.ascontiguousarray(hist_mask, dtype=np.uint8)))
            mask = mask.to(self.device, torch.uint8).contiguous()
            if mask.numel() != n_cand:
                raise ValueError("the history mask has %d bytes for %d candidates" % (mask.numel(), n_cand))
        why_idx = torch.full((max(n, 1), k, m), -1, dtype=torch.int32, device=self.device)
        why_sim = torch.full((max(n, 1), k, m), float("-inf"), dtype=torch.float32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        if n:
            ws = self._grow(self._nbytes("dcue_list_explain_workspace_bytes", n_cand, d, n, k, m))
            nat.check(nat.lib().dcue_list_explain(
                nat.ptr(idx), nat.ptr(count), n, k, nat.ptr(q), nat.ptr(ptr), nat.ptr(hidx), n_rows, nat.ptr(mask),
                nat.ptr(cand_feat), n_cand, d, m, nat.ptr(ws), ws.numel(), nat.ptr(why_idx), nat.ptr(why_sim),
                nat.ptr(flags), nat.stream_handle(self.device)), "dcue_list_explain")
        return why_idx[:n], why_sim[:n], flags[:n]


class TopKMetrics(_Workspace):
    """Precision / Recall / NDCG / MAP / MRR / HitRate at several cutoffs and catalogue coverage of the
    lists of one recommendation setting, computed where dcue_topk leaves them (include/dcue.h
    dcue_topk_metrics / dcue_topk_metrics_mean): no list is copied to the host, no score matrix exists.

    truth_ptr [n_query_rows + 1] int64 / truth_idx int32: per query row, the sorted held-out candidates
    (dcue_topk's exclusion format); excl_ptr / excl_idx, cand_mask, n_cand, score: as TopK, which it owns
    for the lists."""

    def __init__(self, truth_ptr, truth_idx, device, excl_ptr=None, excl_idx=None, cand_mask=None, n_cand=None,
                 score="cosine"):
        self.device = torch.device(device)
        self.topk = TopK(excl_ptr, excl_idx, cand_mask, self.device, n_cand=n_cand, score=score)
        self.cand_mask, self.n_cand = self.topk.cand_mask, self.topk.n_cand
        truth_ptr = np.ascontiguousarray(truth_ptr, dtype=np.int64)
        truth_idx = np.ascontiguousarray(truth_idx, dtype=np.int32)
        if len(truth_ptr) < 2 or truth_ptr[0] != 0 or truth_ptr[-1] != len(truth_idx) or np.any(np.diff(truth_ptr) < 0):
            raise ValueError("truth_ptr is not a CSR pointer array over truth_idx")
        self.n_query_rows = len(truth_ptr) - 1
        if self.topk.excl_ptr is not None and self.topk.excl_ptr.numel() != len(truth_ptr):
            raise ValueError("the exclusion CSR has %d rows, the truth CSR %d"
                             % (self.topk.excl_ptr.numel() - 1, self.n_query_rows))
        self.truth_ptr, self.truth_idx = _upload_csr(truth_ptr, truth_idx, self.device)

    def _cutoffs(self, ks):
        ks = check_cutoffs(ks)
        return ks, (ctypes.c_int32 * len(ks))(*ks)

    def _metrics_into(self, idx, count, q, cut, m, out, flags, exposure):
        """dcue_topk_metrics on device lists, writing out [n, m, 6] / flags [n] (views of the caller's
        buffers) and accumulating into exposure (or None)."""
        nat.check(nat.lib().dcue_topk_metrics(
            nat.ptr(idx), nat.ptr(count), int(q.numel()), int(idx.shape[1]), nat.ptr(q), nat.ptr(self.truth_ptr),
            nat.ptr(self.truth_idx), self.n_query_rows, self.n_cand, ctypes.cast(cut, ctypes.c_void_p), m,
            nat.ptr(out), nat.ptr(flags), nat.ptr(exposure), nat.stream_handle(self.device)), "dcue_topk_metrics")

    def _device_lists(self, idx, count, queries):
        nat.require_gpu(idx, "idx")
        nat.require_gpu(count, "count")
        if idx.dim() != 2 or idx.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() != idx.shape[0]:
            raise ValueError("idx must be int32 [n, k] and count int32 [n]")
        if not 1 <= idx.shape[1] <= nat.TOPK_MAX_K:
            raise ValueError("k must be in 1..%d, got %d" % (nat.TOPK_MAX_K, idx.shape[1]))
        q = torch.as_tensor(np.asarray(queries, dtype=np.int32)).to(self.device)
        if q.numel() != idx.shape[0]:
            raise ValueError("%d queries for %d lists" % (q.numel(), idx.shape[0]))
        return idx.contiguous(), count.contiguous(), q

    def metrics_raw(self, idx, count, queries, ks, exposure=None):
        """(metrics float64 [n, m, 6], flags int32 [n]) device tensors for caller-supplied device lists
        (idx int32 [n, k], count int32 [n], as dcue_topk writes them). exposure: an int32 [m, n_cand]
        device tensor to accumulate into, or None."""
        ks, cut = self._cutoffs(ks)
        idx, count, q = self._device_lists(idx, count, queries)
        if ks[-1] > idx.shape[1]:
            raise ValueError("cutoff %d is beyond the lists' k = %d" % (ks[-1], idx.shape[1]))
        n, m = int(q.numel()), len(ks)
        out = torch.zeros((max(n, 1), m, nat.TOPK_N_METRICS), dtype=torch.float64, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        if n:
            self._metrics_into(idx, count, q, cut, m, out, flags, exposure)
        return out[:n], flags[:n]

    def new_exposure(self, m):
        return torch.zeros((m, self.n_cand), dtype=torch.int32, device=self.device)

    def mean_raw(self, metrics, flags, exposure=None):
        """(mean float64 [m, 6], coverage float64 [m] or None, n_evaluated int32 [1]) device tensors:
        dcue_topk_metrics_mean over metrics [n, m, 6] / flags [n]."""
        n, m = int(metrics.shape[0]), int(metrics.shape[1])
        mean = torch.zeros((m, nat.TOPK_N_METRICS), dtype=torch.float64, device=self.device)
        cov = torch.zeros(m, dtype=torch.float64, device=self.device) if exposure is not None else None
        n_eval = torch.zeros(1, dtype=torch.int32, device=self.device)
        if n == 0:  # (an empty tensor's address may be null)
            metrics = torch.zeros((1, m, nat.TOPK_N_METRICS), dtype=torch.float64, device=self.device)
            flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_topk_metrics_mean(
            nat.ptr(metrics.contiguous()), nat.ptr(flags.contiguous()), n, m, nat.ptr(exposure),
            nat.ptr(self.cand_mask), self.n_cand, nat.ptr(mean), nat.ptr(cov), nat.ptr(n_eval),
            nat.stream_handle(self.device)), "dcue_topk_metrics_mean")
        return mean, cov, n_eval

    def evaluate(self, query_feat, cand_feat, queries, ks, query_batch=None, per_query=False, diversity=None,
                 pool=None, rel=None, ild=False, group_of=None, max_per_group=None, cap_rounds=4, group_stats=False,
                 prior=None, item_value=None, item_tail=None, gini=False):
        """{"ks", "n_evaluated", "precision", "recall", "ndcg", "map", "mrr", "hit", "coverage"}: each
        metric a float64 array over the cutoffs, the mean over the queries with a non-empty truth row;
        per_query adds "per_query" (numpy [n, m, 6], slots in nat.TOPK_METRIC_NAMES order) and "flags".
        Query batches go through TopK.topk_raw with k = max(ks) and dcue_topk_metrics on its device
        tensors; one dcue_topk_metrics_mean call ends it. The result does not depend on query_batch.

        diversity / pool / rel: the lists are TopK.topk_raw's MMR re-ranked ones (k = max(ks)); None
        scores today's lists. ild adds "ild" (float64 over the cutoffs: the mean intra-list diversity
        of the lists that were scored, over those with at least two entries at every cutoff) and
        "n_ild" (their number), by dcue_list_ild / dcue_list_ild_mean on the same device lists.

        group_of / max_per_group / cap_rounds: the lists are TopK.topk_raw's capped ones. group_stats (with
        group_of) adds "group_distinct" and "group_top" (float64 over the cutoffs: the mean number of
        distinct groups in a list's first K entries, and of the most entries one group holds),
        "group_coverage" (the share of the groups that have a candidate which appear in some list's first
        K entries) and "n_group" (the lists behind them), by dcue_list_group_stats /
        dcue_list_group_stats_mean on the same device lists.

        prior: the lists are TopK.topk_raw's with that per-candidate prior (None scores today's lists).
        item_value (float64 [n_cand]) / item_tail (uint8 [n_cand]), either or both: add "novelty" and "tail"
        (float64 over the cutoffs: the mean over the non-empty lists of the first K entries' mean item_value
        -- the self-information gives novelty -- and of their share of tail items; a column that was not
        given is 0) and "n_novelty" (the lists behind them), by dcue_list_item_stats /
        dcue_list_item_stats_mean on the same device lists. gini adds "gini" (float64 over the cutoffs: the
        Gini index of the candidates' exposure in the evaluated lists' first K entries, 0 = every candidate
        served equally often, towards 1 = a few candidates hold all of it), by dcue_exposure_gini on the
        exposure counts coverage is read from.

        Raises ValueError in the evaluator's wording when an eligible candidate's score is NaN or
        infinite, as TopK.topk does."""
        ks, cut = self._cutoffs(ks)
        queries = np.asarray(queries, dtype=np.int64).reshape(-1)
        n, m, k = len(queries), len(ks), ks[-1]
        if diversity is not None or max_per_group is not None:
            check_pool(k, pool)
        elif pool is not None or rel is not None:
            raise ValueError("pool and rel belong to diversity= (pool also to max_per_group=), which is not set")
        cap_kw = {}
        if max_per_group is not None:
            cap_kw = dict(group_of=group_of, max_per_group=max_per_group, cap_rounds=cap_rounds)
        if group_stats:
            g_dev, n_groups, _ = self.topk._group_args(group_of, 1, 1)
            gc = self.topk._cap()
            g_out = torch.zeros((max(n, 1), m, nat.GROUP_N_STATS), dtype=torch.int32, device=self.device)
            g_flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
            g_exposure = gc.new_exposure(m, n_groups)
        pop = None
        if item_value is not None or item_tail is not None or gini:
            pop = PopStats(self.device, self.n_cand, item_value, item_tail)
            p_out = torch.zeros((max(n, 1), m, nat.ITEM_N_STATS), dtype=torch.float64, device=self.device)
            p_flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        if self.topk.excl_ptr is None and query_feat.shape[0] != self.n_query_rows:
            raise ValueError("query factors have %d rows, the truth CSR %d" % (query_feat.shape[0], self.n_query_rows))
        qb = int(self.topk.DEFAULT_QUERY_BATCH if query_batch is None else query_batch)
        if qb < 1:
            raise ValueError("query_batch must be positive")
        out = torch.zeros((max(n, 1), m, nat.TOPK_N_METRICS), dtype=torch.float64, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        nonfinite = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        exposure = self.new_exposure(m)
        if ild:
            div = Diversify(self.device)
            ild_out = torch.zeros((max(n, 1), m), dtype=torch.float64, device=self.device)
            ild_flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        for q0 in range(0, n, qb):
            part = queries[q0:q0 + qb]
            if diversity is None and not cap_kw:
                idx, _, count, tflags = self.topk.topk_raw(query_feat, cand_feat, part, k, query_batch=qb, prior=prior)
            else:
                idx, _, count, tflags = self.topk.topk_raw(query_feat, cand_feat, part, k, query_batch=qb,
                                                           diversity=diversity, pool=pool, rel=rel, prior=prior,
                                                           **cap_kw)
            q = torch.as_tensor(part.astype(np.int32)).to(self.device)
            self._metrics_into(idx, count, q, cut, m, out[q0:], flags[q0:], exposure)
            nonfinite[q0:q0 + len(part)] = tflags
            if ild:
                lists = div._device_lists(idx, count, cand_feat)
                div._ild_into(*lists[:3], ks, cut, ild_out[q0:], ild_flags[q0:])
            if group_stats:
                gc._stats_into(idx.contiguous(), count.contiguous(), g_dev, n_groups, ks, cut, g_out[q0:],
                               g_flags[q0:], g_exposure)
            if pop is not None and (item_value is not None or item_tail is not None):
                pop._stats_into(idx.contiguous(), count.contiguous(), ks, cut, p_out[q0:], p_flags[q0:])
        bad = (nonfinite[:n].cpu().numpy() & 2).astype(bool)
        if bad.any():
            raise self.topk._nonfinite(queries, bad)
        mean, cov, n_eval = self.mean_raw(out[:n], flags[:n], exposure)
        mean = mean.cpu().numpy()
        res = {"ks": list(ks), "n_evaluated": int(n_eval.cpu().numpy()[0])}
        for s, name in enumerate(nat.TOPK_METRIC_NAMES):
            res[name] = mean[:, s].copy()
        res["coverage"] = cov.cpu().numpy()
        if ild:
            ild_mean, n_ild = div.ild_mean_raw(ild_out[:n], ild_flags[:n])
            res["ild"] = ild_mean.cpu().numpy()
            res["n_ild"] = int(n_ild.cpu().numpy()[0])
        if group_stats:
            check_group_flags(queries, g_flags[:n])
            present = torch.zeros(max(n_groups, 1), dtype=torch.uint8, device=self.device)[:n_groups]
            members = g_dev if self.cand_mask is None else g_dev[self.cand_mask != 0]
            present[members[members >= 0].long()] = 1
            g_mean, g_cov, n_g = gc.mean_raw(g_out[:n], g_flags[:n], g_exposure, present)
            g_mean = g_mean.cpu().numpy()
            res.update(group_distinct=g_mean[:, 0].copy(), group_top=g_mean[:, 1].copy(),
                       group_coverage=g_cov.cpu().numpy(), n_group=int(n_g.cpu().numpy()[0]))
        if pop is not None and (item_value is not None or item_tail is not None):
            p_mean, n_p = pop.mean_raw(p_out[:n], p_flags[:n])
            p_mean = p_mean.cpu().numpy()
            res.update(novelty=p_mean[:, 0].copy(), tail=p_mean[:, 1].copy(), n_novelty=int(n_p.cpu().numpy()[0]))
        if gini:
            res["gini"] = pop.gini(exposure, max(n, 1), self.cand_mask)  # (a list names a candidate once)
        if per_query:
            res["per_query"] = out[:n].cpu().numpy()
            res["flags"] = flags[:n].cpu().numpy()
        return res


def histories_csr(rows):
    """int64 pointers / int32 indices of per-row candidate lists, each sorted and without repeats
    (dcue_topk's exclusion CSR, dcue_user_foldin's history CSR)."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    idx = []
    for r, row in enumerate(rows):
        idx.append(np.unique(np.asarray(row, dtype=np.int64)).astype(np.int32))
        ptr[r + 1] = ptr[r] + len(idx[-1])
    return ptr, (np.concatenate(idx) if idx else np.zeros(0, np.int32)).astype(np.int32)


class FoldIn(_Workspace):
    """Device-resident candidate mask and the grow-only workspace of dcue_user_foldin -- TopK's
    counterpart for users outside the trained table: one fresh embedding row per user, learned
    against the frozen towers in one kernel launch for all steps (include/dcue.h).

    cand_mask [n_cand] uint8: the candidates negatives are drawn from (None: every candidate; then
    n_cand must be given)."""

    DEFAULT_USER_BATCH = 4096

    def __init__(self, cand_mask, device, n_cand=None):
        self.device = torch.device(device)
        self.cand_mask, self.n_cand = _upload_mask(cand_mask, n_cand, self.device)

    def workspace_bytes(self, dims, n_users, max_pos, n_neg):
        return self._nbytes("dcue_foldin_workspace_bytes", ctypes.byref(dims), self.n_cand, n_users, max_pos, n_neg)

    def _csr(self, hist_ptr, hist_idx):
        idx = np.ascontiguousarray(hist_idx, dtype=np.int32)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.n_cand):
            raise IndexError("history index out of range")
        return _upload_csr(hist_ptr, idx, self.device)

    @staticmethod
    def config(steps, n_neg, max_pos, margin, lr, beta1, beta2, eps, weight_decay=0.0, seed=0):
        if not 0 <= int(steps) <= nat.FOLDIN_MAX_STEPS:
            raise ValueError("steps must be in 0..%d, got %d" % (nat.FOLDIN_MAX_STEPS, steps))
        if not 1 <= int(n_neg) <= nat.FOLDIN_MAX_NEG:
            raise ValueError("n_neg must be in 1..%d, got %d" % (nat.FOLDIN_MAX_NEG, n_neg))
        if not 1 <= int(max_pos) <= nat.FOLDIN_MAX_POS:
            raise ValueError("max_pos must be in 1..%d, got %d" % (nat.FOLDIN_MAX_POS, max_pos))
        return nat.FoldinConfig(int(steps), int(n_neg), int(max_pos), float(margin), float(lr), float(beta1),
                                float(beta2), float(eps), float(weight_decay), int(seed) & (2 ** 64 - 1))

    def fold_in_raw(self, model, cand_feat, hist_ptr, hist_idx, init, cfg, user_batch=None, row0=0,
                    want_grad=False):
        """(emb [n, E], feat [n, d], loss [n, steps], grad [n, E] or None, flags int32 [n]) device
        tensors, as dcue_user_foldin writes them. model: the nat.Model struct of the frozen towers;
        init [n, E]: the rows' starting values (not modified); hist_ptr / hist_idx: the histories of
        rows row0 .. row0 + n - 1 at those positions of the CSR. Users are passed user_batch at a time
        with their global row, so the result does not depend on user_batch."""
        nat.require_gpu(cand_feat, "cand_feat")
        nat.require_gpu(init, "init")
        cand_feat = cand_feat.contiguous().float()
        d, E = int(model.dims.feature_dim), int(model.dims.user_embdim)
        _check_shapes(cand_feat, self.n_cand, d)
        n = int(init.shape[0])
        if init.dim() != 2 or init.shape[1] != E:
            raise ValueError("init must be [n, %d], got %s" % (E, tuple(init.shape)))
        if len(hist_ptr) < row0 + n + 1:
            raise ValueError("the history CSR has %d rows, %d are needed" % (len(hist_ptr) - 1, row0 + n))
        ptr, idx = self._csr(hist_ptr, hist_idx)
        emb = init.detach().clone().contiguous().float()
        steps = int(cfg.steps)
        feat = torch.zeros((max(n, 1), d), dtype=torch.float32, device=self.device)
        loss = torch.zeros((max(n, 1), max(steps, 1)), dtype=torch.float32, device=self.device)
        grad = torch.zeros((max(n, 1), E), dtype=torch.float32, device=self.device) if want_grad else None
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        ub = int(min(max(n, 1), self.DEFAULT_USER_BATCH if user_batch is None else user_batch))
        if ub < 1:
            raise ValueError("user_batch must be positive")
        ws = self._grow(self.workspace_bytes(model.dims, ub, int(cfg.max_pos), int(cfg.n_neg)))
        for u0 in range(0, n, ub):
            nu = min(ub, n - u0)
            nat.check(nat.lib().dcue_user_foldin(
                ctypes.byref(model), nat.ptr(cand_feat), self.n_cand, nat.ptr(self.cand_mask), nat.ptr(ptr),
                nat.ptr(idx), nu, row0 + u0, ctypes.byref(cfg), ctypes.c_void_p(emb[u0:].data_ptr()), nat.ptr(ws),
                ws.numel(), ctypes.c_void_p(feat[u0:].data_ptr()),
                ctypes.c_void_p(loss[u0:].data_ptr()) if steps else None,
                ctypes.c_void_p(grad[u0:].data_ptr()) if grad is not None else None,
                ctypes.c_void_p(flags[u0:].data_ptr()), nat.stream_handle(self.device)), "dcue_user_foldin")
        return emb[:n], feat[:n], loss[:n, :steps], (grad[:n] if grad is not None else None), flags[:n]

    def negatives(self, hist_ptr, hist_idx, n, cfg, step, row0=0):
        """int32 [n, max_pos, n_neg] device tensor: the negatives dcue_user_foldin draws at `step` for
        rows row0 .. row0 + n - 1 (-1: a dropped slot, or a positive slot the history does not fill)."""
        ptr, idx = self._csr(hist_ptr, hist_idx)
        out = torch.full((max(n, 1), int(cfg.max_pos), int(cfg.n_neg)), -1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_foldin_negatives(self.n_cand, nat.ptr(self.cand_mask), nat.ptr(ptr), nat.ptr(idx),
                                                  int(n), int(row0), ctypes.byref(cfg), int(step), nat.ptr(out),
                                                  nat.stream_handle(self.device)), "dcue_foldin_negatives")
        torch.cuda.synchronize(self.device)  # (ptr / idx are temporaries of this call)
        return out[:n]
