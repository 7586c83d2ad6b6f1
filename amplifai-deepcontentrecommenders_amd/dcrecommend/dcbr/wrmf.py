"""WRMF target factors on the MI355X (BASELINE config 5, the DCBR path).

The reference never published its DCBR package (`dcrecommend/dcbr` is git-ignored, reference
`.gitignore:13`; `nn/dcue_orig.py:35` imports it and fails), so this follows the paper it names:
weighted regularized matrix factorisation for implicit feedback (Hu, Koren, Volinsky, ICDM 2008).
Parity is unpinned against the reference; `oracle/wrmf_oracle.py` (numpy fp64) pins the GPU solver.

Every ALS half-step is one call of `dcue_wrmf_half_step` (csrc/wrmf.hip): the Gram matrix of the
fixed side once, then one workgroup per row builds G + sum (c - 1) f f^T + lambda I in LDS and
solves it by Cholesky. Interactions stay on the device as two CSRs (by user, by item).

Serving: WRMF scores are inner products x_u . y_i, so `recommend`, `recommend_for`
and `evaluate_topk` rank through `dcue_topk_scored(DCUE_SCORE_DOT)` (rank.TopK(score="dot")); `fold_in`
is the closed-form half-step over unseen users' histories; `objective` is the loss the sweeps
descend, from the sparse identity of `dcue_wrmf_objective` (no dense matrix). Everything works on row
indices.
"""
import ctypes

import numpy as np
import torch

from dcrecommend import _native as nat
from dcrecommend.nn import rank


def device_csr(rows, cols, vals, n_rows):
    """(indptr int64 [n_rows + 1], indices int32, values fp32 or None), rows sorted, on rows' device."""
    rows = rows.to(torch.int64)
    order = torch.argsort(rows, stable=True)
    counts = torch.bincount(rows, minlength=n_rows)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    indptr[1:] = torch.cumsum(counts, 0)
    indices = cols[order].to(torch.int32).contiguous()
    values = None if vals is None else vals[order].to(torch.float32).contiguous()
    return indptr, indices, values


class WRMF:
    """Implicit-feedback ALS: confidence c = 1 + alpha * v on the observed pairs (v = play counts,
    or 1), preference 1 there and 0 elsewhere, L2 weight `regularization` on both factor sets.

    `fit(user_idx, item_idx, values=None)` runs `iterations` sweeps (users, then items) and leaves
    `user_factors` [n_users, factors] and `item_factors` [n_items, factors] on the device.

    Data parallelism (comm: a distributed.NativeComm / HostComm): every rank holds the whole
    interaction set and both factor matrices; a half-step solves this rank's contiguous 1/world of
    the rows (rows are independent, so each is solved exactly as on one GPU) and an in-place
    all-gather (dcue_comm_allgather) hands every rank all of them before the next half-step. The
    factor matrices are kept padded to a multiple of world rows (the pad rows have no pairs: 0)."""

    def __init__(self, factors=128, regularization=0.01, alpha=40.0, iterations=15, seed=0, device="cuda",
                 comm=None):
        if not 1 <= int(factors) <= 128:
            raise ValueError("factors must be in [1, 128] (the per-row solve holds a factors^2 matrix in LDS)")
        if not regularization > 0:
            raise ValueError("regularization must be > 0")
        self.factors, self.regularization, self.alpha = int(factors), float(regularization), float(alpha)
        self.iterations, self.seed, self.device = int(iterations), int(seed), torch.device(device)
        self.user_factors = self.item_factors = None
        self._ws = None
        self.comm = comm
        self.world = comm.world if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        self._uf = self._if = None  # the padded storage behind user_factors / item_factors
        self._obj_ws = None
        self._serve = {}  # per fit: the sorted exclusion CSR and the TopK objects over it

    def _workspace(self, n_fixed):
        nbytes = ctypes.c_size_t()
        nat.check(nat.lib().dcue_wrmf_workspace_bytes(self.factors, int(n_fixed), ctypes.byref(nbytes)),
                  "dcue_wrmf_workspace_bytes")
        if self._ws is None or self._ws.numel() < nbytes.value:
            self._ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        return self._ws

    def half_step(self, solve, fixed, csr):
        """solve[r] <- the WRMF least-squares solution of row r with `fixed` held (in place). Under a
        communicator, `solve` is a view of padded storage (user_factors / item_factors): this rank
        solves its part of the rows, then every rank gathers the others'."""
        indptr, indices, values = csr
        if indptr.numel() != solve.shape[0] + 1:
            raise ValueError("the CSR has %d rows, the solved factors %d" % (indptr.numel() - 1, solve.shape[0]))
        if solve.shape[1] != self.factors or fixed.shape[1] != self.factors:
            raise ValueError("factor matrices must be [n, %d]" % self.factors)
        ws = self._workspace(fixed.shape[0])
        n = solve.shape[0]
        per = (n + self.world - 1) // self.world
        r0, r1 = min(n, self.rank * per), min(n, (self.rank + 1) * per)
        if r1 > r0:
            nat.check(nat.lib().dcue_wrmf_half_step(
                nat.ptr(solve[r0:r1]), r1 - r0, nat.ptr(fixed), fixed.shape[0], self.factors,
                nat.ptr(indptr[r0:]), nat.ptr(indices), nat.ptr(values), self.alpha, self.regularization,
                nat.ptr(ws), ws.numel(), nat.stream_handle()), "dcue_wrmf_half_step")
        if self.world > 1:
            full = self._storage(solve)
            self.comm.allgather_(full[:per * self.world].view(-1))
        return solve

    def _storage(self, view):
        for buf in (self._uf, self._if):
            if buf is not None and view.data_ptr() == buf.data_ptr():
                return buf
        raise ValueError("under a communicator, half_step solves user_factors or item_factors in place")

    def init_factors(self, n_users, n_items):
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        uf = (torch.randn(n_users, self.factors, generator=g) * 0.01).to(self.device)
        itf = (torch.randn(n_items, self.factors, generator=g) * 0.01).to(self.device)
        w = self.world
        self._uf = torch.zeros(((n_users + w - 1) // w) * w, self.factors, device=self.device)
        self._if = torch.zeros(((n_items + w - 1) // w) * w, self.factors, device=self.device)
        self._uf[:n_users].copy_(uf)
        self._if[:n_items].copy_(itf)
        self.user_factors, self.item_factors = self._uf[:n_users], self._if[:n_items]

    def fit(self, user_idx, item_idx, values=None, n_users=None, n_items=None, tol=None, track_objective=False):
        """track_objective: `objective_history` gets L (objective()) after each iteration. tol: the
        sweeps stop once an iteration lowers L by less than tol * |L| (implies the tracking). With the
        defaults no objective is computed and exactly `iterations` sweeps run."""
        u = torch.as_tensor(user_idx, device=self.device)
        i = torch.as_tensor(item_idx, device=self.device)
        v = None if values is None else torch.as_tensor(values, device=self.device)
        n_users = int(u.max()) + 1 if n_users is None else int(n_users)
        n_items = int(i.max()) + 1 if n_items is None else int(n_items)
        # every index is a row of the other side's factors: the solver gathers them unchecked
        if int(u.min()) < 0 or int(u.max()) >= n_users or int(i.min()) < 0 or int(i.max()) >= n_items:
            raise ValueError("user / item indices must lie in [0, n_users) / [0, n_items)")
        self.by_user = device_csr(u, i, v, n_users)
        self.by_item = device_csr(i, u, v, n_items)
        # (re)initialise unless both factor sets already have this problem's shapes (a refit with a
        # different item count must not keep item factors the CSRs index past)
        if (self.user_factors is None or self.user_factors.shape[0] != n_users
                or self.item_factors.shape[0] != n_items):
            self.init_factors(n_users, n_items)
        self._serve = {}
        self.objective_history = []
        for _ in range(self.iterations):
            self.half_step(self.user_factors, self.item_factors, self.by_user)
            self.half_step(self.item_factors, self.user_factors, self.by_item)
            if track_objective or tol is not None:
                self.objective_history.append(self.objective())
                h = self.objective_history
                if tol is not None and len(h) > 1 and h[-2] - h[-1] < float(tol) * abs(h[-2]):
                    break
        return self

    # ------------------------------------------------------------------ the objective
    def objective_terms(self):
        """(L, observed term, all-pairs term, regulariser) of include/dcue.h dcue_wrmf_objective: the
        objective of loss(), in fp64 from the sparse identity -- the observed pairs and two Gram
        matrices, never the [users][items] matrix."""
        X, Y = self.user_factors, self.item_factors
        indptr, indices, values = self.by_user
        nbytes = ctypes.c_size_t()
        nat.check(nat.lib().dcue_wrmf_objective_workspace_bytes(X.shape[0], Y.shape[0], self.factors,
                                                                ctypes.byref(nbytes)),
                  "dcue_wrmf_objective_workspace_bytes")
        if self._obj_ws is None or self._obj_ws.numel() < nbytes.value:
            self._obj_ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        out = torch.zeros(4, dtype=torch.float64, device=self.device)
        if indices.numel() == 0:  # (an empty tensor's address may be null)
            indices = torch.zeros(1, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().dcue_wrmf_objective(
            nat.ptr(X), X.shape[0], nat.ptr(Y), Y.shape[0], self.factors, nat.ptr(indptr), nat.ptr(indices),
            nat.ptr(values), self.alpha, self.regularization, nat.ptr(self._obj_ws), self._obj_ws.numel(),
            nat.ptr(out), nat.stream_handle()), "dcue_wrmf_objective")
        return tuple(float(v) for v in out.cpu())

    def objective(self):
        """The WRMF objective L as a float, at any scale (loss() is its dense restatement)."""
        return self.objective_terms()[0]

    # ------------------------------------------------------------------ serving
    def _seen(self):
        """by_user as dcue_topk's exclusion CSR: each row sorted, no repeats (device tensors)."""
        if "seen" not in self._serve:
            indptr, indices, _ = self.by_user
            n_users, n_items = indptr.numel() - 1, self.item_factors.shape[0]
            rows = torch.repeat_interleave(torch.arange(n_users, device=indptr.device), indptr[1:] - indptr[:-1])
            key = torch.unique(rows * n_items + indices.long())  # (sorted)
            ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=indptr.device)
            ptr[1:] = torch.cumsum(torch.bincount(key // n_items, minlength=n_users), 0)
            self._serve["seen"] = (ptr, (key % n_items).to(torch.int32))
        return self._serve["seen"]

    def _candidates(self, item_factors):
        cand = self.item_factors if item_factors is None else item_factors
        nat.require_gpu(cand, "item_factors")
        if cand.dim() != 2 or cand.shape[1] != self.factors:
            raise ValueError("item factors must be [n, %d], got %s" % (self.factors, tuple(cand.shape)))
        return cand

    @staticmethod
    def _mask(cand_mask):
        return cand_mask.cpu().numpy() if torch.is_tensor(cand_mask) else cand_mask

    def _topk(self, exclude_seen, cand_mask, n_cand):
        """rank.TopK(score="dot") over the fit's exclusion rows; the mask-free ones are kept (their
        workspace with them)."""
        ptr, idx = self._seen() if exclude_seen else (None, None)
        if cand_mask is not None:
            return rank.TopK(ptr, idx, self._mask(cand_mask), self.device, score="dot")
        key = ("topk", bool(exclude_seen), n_cand)
        if key not in self._serve:
            self._serve[key] = rank.TopK(ptr, idx, None, self.device, n_cand=n_cand, score="dot")
        return self._serve[key]

    def recommend(self, users, k=10, exclude_seen=True, item_factors=None, cand_mask=None, diversity=None,
                  pool=None, groups=None, max_per_group=None, item_prior=None):
        """The k best items for each user row by x_u . y_i: (idx int64 [n, k], score float32 [n, k],
        count int32 [n]) numpy arrays, best first, short lists padded with -1 / -inf. exclude_seen
        drops the items of the user's by_user row. item_factors [n_cand, factors] (device) replaces
        the candidate table (DCBR.hybrid_item_factors: predicted factors for cold items); cand_mask
        [n_cand]: 0 = never return the item. One fused GPU pass (include/dcue.h dcue_topk_scored).

        diversity (lambda in [0, 1]; None: the plain ranking): the user's `pool` best items (default
        min(128, 4 k)) re-ranked down to k by Maximal Marginal Relevance (dcue_list_mmr) -- the
        inner-product scores min-max scaled per list, the redundancy the cosine of the candidate
        factors, as similar_items measures it. The lists are then in selection order, each entry
        with its own inner-product score.

        max_per_group with groups, an int array by candidate row (an item's artist, album, ...; -1: none):
        no group holds more than that many items of a list (rank.TopK.topk_raw max_per_group=:
        dcue_list_group_cap on the `pool` best items, short lists ranked deeper; with diversity= the
        pool is capped before MMR picks from it).

        item_prior (None: the plain inner product): a finite float array by candidate row added to every
        score of its item inside the fused ranking (dcue_topk_prior) -- item biases, a popularity
        correction, boosts; the scores returned are the sums, and the prior reaches every ranking the call
        makes (the pool of diversity=, each round of max_per_group=)."""
        cand = self._candidates(item_factors)
        if exclude_seen and cand.shape[0] != self.item_factors.shape[0]:
            raise ValueError("exclude_seen needs a candidate table with the fit's %d items" % self.item_factors.shape[0])
        tk = self._topk(exclude_seen, cand_mask, int(cand.shape[0]))
        return tk.topk(self.user_factors, cand, np.asarray(users, dtype=np.int64).reshape(-1), k,
                       diversity=diversity, pool=pool, prior=item_prior, **self._group_kw(groups, max_per_group))

    @staticmethod
    def _group_kw(groups, max_per_group):
        """rank.TopK's group arguments (none without a cap: today's path)."""
        if max_per_group is None:
            if groups is not None:
                raise ValueError("groups goes with max_per_group=, which is not set")
            return {}
        return dict(group_of=groups, max_per_group=max_per_group)

    def explain(self, users, k=10, reasons=3, exclude_seen=True, item_factors=None, cand_mask=None, diversity=None,
                pool=None, item_prior=None):
        """recommend()'s lists with the reason for every pick: (idx, score, count) as recommend() returns
        them (the same dcue_topk_scored call) plus why_idx int64 [n, k, reasons] / why_sim float32
        [n, k, reasons] -- per pick the `reasons` (1..8) items of the user's by_user row nearest to it by
        the cosine of the candidate factors, the score similar_items reports for the pair (include/dcue.h
        dcue_list_explain, on the device lists); short rows end in -1 / -inf. The candidate table must
        have the fit's items. item_prior: as recommend()."""
        reasons = rank.check_reasons(reasons)
        cand = self._candidates(item_factors)
        if cand.shape[0] != self.item_factors.shape[0]:
            raise ValueError("explain needs a candidate table with the fit's %d items" % self.item_factors.shape[0])
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        tk = self._topk(exclude_seen, cand_mask, int(cand.shape[0]))
        idx, score, count, flags = tk.topk_raw(self.user_factors, cand, users, k, diversity=diversity, pool=pool,
                                               prior=item_prior)
        bad = (flags.cpu().numpy() & 2).astype(bool)
        if bad.any():
            raise tk._nonfinite(users, bad)
        if "explain" not in self._serve:
            self._serve["explain"] = rank.Explain(self.device)
        why_idx, why_sim, eflags = self._serve["explain"].explain_raw(idx, count, users, *self._seen(), cand, reasons)
        rank.check_explain_flags(users, eflags)
        return (idx.cpu().numpy().astype(np.int64), score.cpu().numpy(), count.cpu().numpy(),
                why_idx.cpu().numpy().astype(np.int64), why_sim.cpu().numpy())

    def similar_items(self, items, k=10):
        """The k items most similar to each item row, by the cosine of the item factors (dcue_topk, as
        DCUE.similar_songs), each item excluded from its own list; same return as recommend()."""
        Y = self.item_factors
        if "similar" not in self._serve:
            self._serve["similar"] = rank.TopK(*rank.identity_csr(Y.shape[0]), None, self.device, n_cand=Y.shape[0])
        return self._serve["similar"].topk(Y, Y, np.asarray(items, dtype=np.int64).reshape(-1), k)

    def _histories(self, histories, values):
        """(indptr, indices, values or None) device tensors of the histories in their own order
        (repeats kept: the half-step sums them), after the index check."""
        n_items = self.item_factors.shape[0]
        if values is not None and len(values) != len(histories):
            raise ValueError("%d value lists for %d histories" % (len(values), len(histories)))
        rows = [np.asarray(h, dtype=np.int64).reshape(-1) for h in histories]
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= n_items):
            raise ValueError("history item indices must lie in [0, %d)" % n_items)
        val = None
        if values is not None:
            vals = [np.asarray(v, dtype=np.float32).reshape(-1) for v in values]
            if [len(v) for v in vals] != [len(r) for r in rows]:
                raise ValueError("values must match the histories item for item")
            val = np.concatenate(vals) if vals else np.zeros(0, np.float32)
            val = torch.from_numpy(val if len(val) else np.zeros(1, np.float32)).to(self.device)
        idx = idx.astype(np.int32) if len(idx) else np.zeros(1, np.int32)
        return torch.from_numpy(ptr).to(self.device), torch.from_numpy(idx).to(self.device), val

    def fold_in(self, histories, values=None):
        """User factors [n, factors] (device) for users outside the fit, each given as a list of item
        rows (values: the matching play counts; default 1): the closed-form WRMF solution against the
        fixed item factors -- one dcue_wrmf_half_step over the histories' CSR, exactly the row a
        refit's user half-step would give. No row of user_factors is written. An empty history gives
        a zero row; an item index outside [0, n_items) raises ValueError. Under a communicator every
        rank solves every history (nothing is gathered)."""
        Y = self.item_factors
        indptr, indices, val = self._histories(histories, values)
        n = len(histories)
        out = torch.zeros((n, self.factors), dtype=torch.float32, device=self.device)
        if n:
            ws = self._workspace(Y.shape[0])
            nat.check(nat.lib().dcue_wrmf_half_step(
                nat.ptr(out), n, nat.ptr(Y), Y.shape[0], self.factors, nat.ptr(indptr), nat.ptr(indices),
                nat.ptr(val), self.alpha, self.regularization, nat.ptr(ws), ws.numel(), nat.stream_handle()),
                "dcue_wrmf_half_step")
            torch.cuda.current_stream().synchronize()  # (indptr / indices / val are temporaries of this call)
        return out

    def recommend_for(self, histories, k=10, exclude_history=True, values=None, item_factors=None, cand_mask=None,
                      diversity=None, pool=None, groups=None, max_per_group=None, item_prior=None):
        """recommend() for users outside the fit: fold_in(histories, values), then the inner-product
        top-k with each history as the user's exclusion row. diversity / pool / groups / max_per_group /
        item_prior: as recommend(). Returns what recommend() returns."""
        cand = self._candidates(item_factors)
        feat = self.fold_in(histories, values)
        ptr, idx = rank.histories_csr(histories) if exclude_history else (None, None)
        tk = rank.TopK(ptr, idx, self._mask(cand_mask), self.device, n_cand=int(cand.shape[0]), score="dot")
        return tk.topk(feat, cand, np.arange(len(histories)), k, diversity=diversity, pool=pool, prior=item_prior,
                       **self._group_kw(groups, max_per_group))

    def evaluate_topk(self, truth_ptr, truth_idx, ks=(10, 50, 100), users=None, exclude_ptr=None, exclude_idx=None,
                      item_factors=None, cand_mask=None, per_user=False, diversity=None, pool=None, ild=False,
                      groups=None, max_per_group=None, item_prior=None, item_value=None, item_tail=None, gini=False):
        """Top-K ranking quality of the inner-product lists against held-out truth rows (a CSR over
        user rows, each row sorted, no repeats): DCUE.evaluate_topk's dict -- {"precision@K",
        "recall@K", "ndcg@K", "map@K", "mrr@K", "hit@K", "coverage@K" for each K of ks, "n_users"} --
        through rank.TopKMetrics(score="dot"). users: user rows (default: every row with truth);
        exclude_ptr / exclude_idx: what the lists must not return (the training interactions;
        default none); per_user adds "users", "per_user" and "flags". diversity / pool: score
        recommend(diversity=, pool=)'s MMR re-ranked lists (k = max(ks)) instead; ild adds "ild@K" (the
        mean intra-list diversity of the scored lists, dcue_list_ild) and "n_ild". groups (an int array by
        candidate row) adds "groups@K", "group_top@K" and "group_coverage@K" -- DCUE.evaluate_topk's
        artist numbers (dcue_list_group_stats) -- and "n_group_lists"; with max_per_group the lists scored
        are recommend(groups=, max_per_group=)'s.

        item_prior: score recommend(item_prior=)'s lists. item_value (float64 by candidate row, e.g. the
        items' self-information) / item_tail (uint8, non-zero = long tail) add "novelty@K" and "tail@K" (the
        mean over the lists of the first K items' mean value and tail share, dcue_list_item_stats) and
        "n_novelty"; gini adds "gini@K", the Gini index of the candidates' exposure (dcue_exposure_gini).
        The caller supplies the arrays: this path has no dataset to take play counts from."""
        ks = rank.check_cutoffs(ks)
        cand = self._candidates(item_factors)
        ev = rank.TopKMetrics(truth_ptr, truth_idx, self.device, excl_ptr=exclude_ptr, excl_idx=exclude_idx,
                              cand_mask=self._mask(cand_mask), n_cand=int(cand.shape[0]), score="dot")
        if users is None:
            rows = np.flatnonzero(np.diff(np.asarray(truth_ptr, dtype=np.int64)) > 0).astype(np.int64)
        else:
            rows = np.asarray(users, dtype=np.int64).reshape(-1)
        group_kw = {} if groups is None else dict(group_of=groups, group_stats=True)
        if max_per_group is not None:
            group_kw.update(self._group_kw(groups, max_per_group))
        res = ev.evaluate(self.user_factors, cand, rows, ks, per_query=per_user, diversity=diversity, pool=pool,
                          ild=ild, prior=item_prior, item_value=item_value, item_tail=item_tail, gini=gini, **group_kw)
        out = {"n_users": res["n_evaluated"]}
        if groups is not None:
            for name, slot in (("groups", "group_distinct"), ("group_top", "group_top"),
                               ("group_coverage", "group_coverage")):
                for i, k in enumerate(ks):
                    out["%s@%d" % (name, k)] = float(res[slot][i])
            out["n_group_lists"] = res["n_group"]
        for name in nat.TOPK_METRIC_NAMES + ("coverage",) + (("ild",) if ild else ()):
            for i, k in enumerate(ks):
                out["%s@%d" % (name, k)] = float(res[name][i])
        if ild:
            out["n_ild"] = res["n_ild"]
        pop_names = (("novelty", "tail") if "novelty" in res else ()) + (("gini",) if gini else ())
        for name in pop_names:
            for i, k in enumerate(ks):
                out["%s@%d" % (name, k)] = float(res[name][i])
        if "novelty" in res:
            out["n_novelty"] = res["n_novelty"]
        if per_user:
            out.update(users=rows.tolist(), per_user=res["per_query"], flags=res["flags"])
        return out

    def loss(self):
        """The WRMF objective sum_{u,i} c_ui (p_ui - x_u.y_i)^2 + lambda (|X|^2 + |Y|^2), evaluated
        in fp64 from the dense score matrix (small problems: diagnostics and tests)."""
        X, Y = self.user_factors.double(), self.item_factors.double()
        S = X @ Y.T
        indptr, indices, values = self.by_user
        rows = torch.repeat_interleave(torch.arange(X.shape[0], device=X.device), indptr[1:] - indptr[:-1])
        C = torch.ones_like(S)
        P = torch.zeros_like(S)
        vv = torch.ones(indices.shape[0], dtype=torch.float64, device=X.device) if values is None else values.double()
        C[rows, indices.long()] = 1.0 + self.alpha * vv
        P[rows, indices.long()] = 1.0
        return float((C * (P - S) ** 2).sum() + self.regularization * ((X ** 2).sum() + (Y ** 2).sum()))
