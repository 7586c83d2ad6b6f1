"""dcue_select_negatives and the trainer path over it against the definition in
hard_negatives_reference.py (numpy, fp64 scores).

Table: 3,000 items and 300 users of randn factors, 700 rows, pools from randint(0, 3000): duplicates
occur. The fp32 kernel may order two candidates the other way round only where their fp64 cosines are
closer than tau = 4 max(d, 32) 2^-24 -- three fp32 sums of at most d_s terms each, two scores compared,
a relative rounding of 2^-24 per operation; derived, not measured. Every row is held to it
(check_against): h exact, the hard positions ascending, eligible and within tau of the boundary score,
no unchosen eligible position above it by more than tau, the fill exactly the definition's. Where the
boundary gap is at least tau that is equality with the reference, which is nearly every row."""
import functools
import os
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

import hard_negatives_reference as R
import weighted_sampler_reference as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ITEMS, N_USERS, N_ROWS = 3000, 300, 700
DS = (1, 30, 100, 128, 256)
PS = (1, 21, 67, 160, 1024)


@functools.lru_cache(maxsize=None)
def _factors(d):
    rs = np.random.RandomState(1000 + d)
    uf, itf = rs.randn(N_USERS, d).astype(np.float32), rs.randn(N_ITEMS, d).astype(np.float32)
    uf.setflags(write=False)
    itf.setflags(write=False)
    return uf, itf


@functools.lru_cache(maxsize=None)
def _rows(P):
    rs = np.random.RandomState(2000 + P)
    pool = rs.randint(0, N_ITEMS, (N_ROWS, P)).astype(np.int64)
    users = rs.randint(0, N_USERS, N_ROWS).astype(np.int64)
    pool.setflags(write=False)
    users.setflags(write=False)
    return users, pool


@functools.lru_cache(maxsize=None)
def _table(d, P):
    """The fp64 scores of every row: computed once per (d, P), shared and left unchanged."""
    uf, itf = _factors(d)
    users, pool = _rows(P)
    return R.score_table(uf, itf, users, pool)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared arrays are read-only


def _select(uf, itf, users, pool, N, H):
    """One call on device tensors: numpy (out, hard, flags). The outputs start as a sentinel, so a
    word the kernel left unwritten shows."""
    from dcrecommend import _native as nat
    n = users.numel()
    out = torch.full((n, N), -7, dtype=torch.int64, device=DEV)
    hard = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    nat.select_negatives(uf, itf, users, pool, N, H, out, hard, flags)
    return out.cpu().numpy(), hard.cpu().numpy(), flags.cpu().numpy()


def _shapes(P):
    """(N, H) with N in {1, 20, P}, N <= P, and H in {0, 1, N // 2, N}."""
    return [(N, H) for N in sorted({n for n in (1, 20, P) if n <= P}) for H in sorted({0, 1, N // 2, N}) if H <= N]


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("d", DS)
def test_selection_within_tau_of_the_definition(d, P):
    uf, itf = _factors(d)
    users, pool = _rows(P)
    table = _table(d, P)
    duf, ditf, dusers, dpool = _dev(uf), _dev(itf), _dev(users), _dev(pool)
    assert P < 67 or any(len(np.unique(r)) < P for r in pool)  # duplicates do occur
    exact = total = 0
    for N, H in _shapes(P):
        for n in (1, N_ROWS):
            out, hard, flags = _select(duf, ditf, dusers[:n], dpool[:n], N, H)
            assert (flags == 0).all()
            exact += R.check_against(uf, itf, users[:n], pool[:n], N, H, out, hard, table=table[:n])
            total += n
            if H == 0:
                assert np.array_equal(out, pool[:n, :N]) and (hard == 0).all()
    if d >= 100:  # the issue's CPU run of the reference: at most 1.4 % of rows with a gap below 2 tau
        assert exact >= 0.95 * total, (exact, total)


@pytest.mark.parametrize("d", [30, 100, 256])
def test_batching_does_not_change_a_bit(d):
    """The 700 rows in one call, and the same rows in calls of 1, 63 and 636: identical outputs."""
    uf, itf = _factors(d)
    users, pool = _rows(160)
    duf, ditf, dusers, dpool = _dev(uf), _dev(itf), _dev(users), _dev(pool)
    whole = _select(duf, ditf, dusers, dpool, 20, 10)
    parts, b0 = [], 0
    for n in (1, 63, 636):
        parts.append(_select(duf, ditf, dusers[b0:b0 + n].contiguous(), dpool[b0:b0 + n].contiguous(), 20, 10))
        b0 += n
    assert b0 == N_ROWS
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), k
    # and a row's choice does not depend on where it stands in the batch
    again = _select(duf, ditf, dusers.flip(0).contiguous(), dpool.flip(0).contiguous(), 20, 10)
    for k in range(3):
        assert np.array_equal(whole[k], again[k][::-1]), k


def _exact_case(d=30):
    rs = np.random.RandomState(7)
    uf = rs.randn(4, d).astype(np.float32)
    itf = rs.randn(40, d).astype(np.float32)
    uf[1] = 0                  # a zero user row
    itf[10:20] = itf[0:10]     # ids 10..19 are bitwise copies of ids 0..9
    itf[25, d // 2] = np.nan   # a NaN item row
    return uf, itf


@pytest.mark.parametrize("d", [1, 30, 100, 256])
def test_exact_cases(d):
    uf, itf = _exact_case(d)
    n_items = len(itf)
    duf, ditf = _dev(uf), _dev(itf)

    def run(users, pool, N, H):
        users, pool = np.asarray(users, dtype=np.int64), np.asarray(pool, dtype=np.int64)
        got = _select(duf, ditf, _dev(users), _dev(pool), N, H)
        want = R.select(uf, itf, users, pool, N, H)
        return got, want

    # bitwise-equal item rows tie, and the tie goes to the earlier position: pools of one row's copies
    # (i, i + 10) in either order, with one more distinct item behind them
    pool = [[i, i + 10, 30] for i in range(10)] + [[i + 10, i, 30] for i in range(10)]
    (out, hard, flags), want = run([0] * 20, pool, 2, 1)
    s = R.cosines(uf[0], itf)
    for r, row in enumerate(pool):
        # the pair outranks item 30 (a tie goes to the earlier position too), or item 30 is the hard one
        first_wins = s[row[0]] >= s[30]
        assert out[r].tolist() == ([row[0], row[1]] if first_wins else [30, row[0]]), r
    assert (hard == 1).all() and (flags == 0).all() and np.array_equal(out, want[0])

    # a zero user row: every score is 0, the hard set is the first h first occurrences
    pool = [[5, 5, 3, 9, 3, 7, 1, 5], [2, 2, 2, 2, 2, 2, 2, 4]]
    (out, hard, flags), _ = run([1, 1], pool, 5, 3)
    assert out.tolist() == [[5, 3, 9, 5, 3], [2, 4, 2, 2, 2]] and hard.tolist() == [3, 2] and flags.tolist() == [0, 0]

    # a NaN item row is never hard and sets bit 1
    (out, hard, flags), want = run([0, 0, 2], [[25, 25, 25], [25, 1, 2], [1, 2, 3]], 3, 3)
    assert out.tolist() == [[25, 25, 25], [1, 2, 25], [1, 2, 3]] and hard.tolist() == [0, 2, 3]
    assert flags.tolist() == [1, 1, 0]

    # -1 and n_items are never hard, set bit 2 and pass through the fill
    (out, hard, flags), want = run([0, 2, 3], [[-1, n_items, 4, 6], [-1, -1, n_items, n_items], [6, 4, 2, 0]], 4, 4)
    assert out[0].tolist() == [4, 6, -1, n_items] and out[1].tolist() == [-1, -1, n_items, n_items]
    assert hard.tolist() == [2, 0, 4] and flags.tolist() == [2, 2, 0]
    for g, w in zip((out, hard, flags), want):
        assert np.array_equal(g, w)
    (out, hard, flags), _ = run([0], [[n_items + 10 ** 12, -2 ** 40, 3, 3]], 2, 2)  # far outside: never addressed
    assert out.tolist() == [[3, n_items + 10 ** 12]] and hard.tolist() == [1] and flags.tolist() == [2]

    # a user id outside the table: bit 2 and h = 0
    (out, hard, flags), _ = run([-1, 4, 2 ** 40], [[3, 2, 1], [1, 2, 3], [2, 2, 2]], 2, 2)
    assert out.tolist() == [[3, 2], [1, 2], [2, 2]] and hard.tolist() == [0, 0, 0] and flags.tolist() == [2, 2, 2]

    # a pool of one repeated id gives h = 1
    for P in (1, 64, 257, 1024):
        (out, hard, flags), _ = run([0, 2], [[8] * P, [31] * P], min(P, 20), min(P, 20))
        assert (out[0] == 8).all() and (out[1] == 31).all() and hard.tolist() == [1, 1] and flags.tolist() == [0, 0]

    # H = 0 returns pool[:, :N]
    rs = np.random.RandomState(d)
    pool = rs.randint(-1, n_items + 1, (50, 67))
    (out, hard, flags), want = run(rs.randint(0, 4, 50), pool, 20, 0)
    assert np.array_equal(out, pool[:, :20]) and (hard == 0).all() and np.array_equal(flags, want[2])


def test_every_position_can_be_hard_at_the_largest_pool():
    """P = N = H = 1024 over distinct ids: all four thread slots, every wave of the compaction."""
    uf, itf = _factors(100)
    rs = np.random.RandomState(11)
    pool = np.stack([rs.permutation(N_ITEMS)[:1024] for _ in range(3)]).astype(np.int64)
    users = np.array([0, 1, 2], dtype=np.int64)
    out, hard, flags = _select(_dev(uf), _dev(itf), _dev(users), _dev(pool), 1024, 1024)
    assert np.array_equal(out, pool) and hard.tolist() == [1024] * 3 and flags.tolist() == [0] * 3
    out, hard, flags = _select(_dev(uf), _dev(itf), _dev(users), _dev(pool), 1024, 512)
    R.check_against(uf, itf, users, pool, 1024, 512, out, hard)


def test_wrapper_validation():
    from dcrecommend import _native as nat
    uf, itf = _factors(30)
    users, pool = _rows(21)
    duf, ditf, dusers, dpool = _dev(uf), _dev(itf), _dev(users[:4]), _dev(pool[:4])
    launches = nat.lib().dcue_launch_count()
    for N, H in ((0, 0), (22, 1), (20, 21), (20, -1)):
        with pytest.raises(RuntimeError, match="DCUE_ERR_INVALID"):
            nat.select_negatives(duf, ditf, dusers, dpool, N, H)
    wide = torch.zeros((4, 257), device=DEV)
    with pytest.raises(RuntimeError, match="DCUE_ERR_UNSUPPORTED"):
        nat.select_negatives(wide, wide, dusers, dpool, 20, 10)
    with pytest.raises(ValueError):
        nat.select_negatives(duf.double(), ditf, dusers, dpool, 20, 10)
    with pytest.raises(ValueError):
        nat.select_negatives(duf, ditf[:, :20], dusers, dpool, 20, 10)
    with pytest.raises(ValueError):
        nat.select_negatives(duf, ditf, dusers.int(), dpool, 20, 10)
    out, hard, flags = nat.select_negatives(duf, ditf, dusers[:0], dpool[:0], 20, 10)
    assert out.shape == (0, 20) and hard.numel() == 0 and flags.numel() == 0
    assert nat.lib().dcue_launch_count() == launches


# ------------------------------------------------------------------------------------- trainer
def _frames(g, tmp_path):
    """tests/golden/eval.npz's triplets (30 users x 48 songs, the golden fit's set) and metadata, as
    tests/test_gpu_weighted_sampler.py builds them."""
    trip = pd.DataFrame({"user_id": g["raw_users"], "song_id": g["raw_songs"], "score": g["raw_score"]})
    paths = [""] * len(g["meta_songs"])
    for k in range(len(paths)):
        paths[k] = os.path.join(str(tmp_path), "m%03d.pt" % k)
        if not os.path.exists(paths[k]):
            torch.save(torch.from_numpy(g["spec"][k].astype(np.float32)), paths[k])
    meta = pd.DataFrame({"idx": np.arange(len(paths)), "song_id": g["meta_songs"], "data_mel": paths})
    return trip, meta


N_NEG = 3


def _trainer(golden, tmp_path, factors=True, ds_kw=None, **kw):
    """A fresh trainer over eval.npz's train split, seeded, ready for one sub-epoch: (trainer, dataset,
    loader)."""
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    from dcrecommend.nn.dcue import DCUE
    trip, meta = _frames(golden("eval.npz"), tmp_path)
    ds = DCUEDataset(trip.copy(), meta, neg_samples=N_NEG, split="train", **(ds_kw or {}))
    items = DCUEItemset(trip.copy(), meta)
    tr = DCUE(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=N_NEG, lr=1e-3, device=DEV, **kw)
    tr.n_users, tr.n_items, tr.epoch_size = len(ds.user_index), len(ds.item_index), 64
    tr.train_data = ds
    np.random.seed(13)
    torch.manual_seed(13)
    tr._init_nn()
    tr._bind_items(items)
    if factors:
        tr._user_factors(items)
        tr._item_factors(items)
    np.random.seed(14)
    torch.manual_seed(14)
    loader = tr._batch_loaders(ds, k=10)[0]
    tr.scheduler.step()
    return tr, ds, loader


def _params(tr):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


def test_pool_of_n_without_hard_is_the_plain_sampler(golden, tmp_path):
    """neg_pool=N, neg_hard=0: the parameters bit for bit, the loss and numpy's stream position of
    neg_pool=None."""
    state = np.random.get_state()
    try:
        runs = []
        for kw in ({}, dict(neg_pool=N_NEG, neg_hard=0)):
            tr, ds, loader = _trainer(golden, tmp_path, **kw)
            res = tr._train_epoch(loader)
            runs.append((res, _params(tr), int(np.random.randint(0, 2 ** 31)), int(torch.randint(0, 2 ** 31, ()))))
        (res_a, par_a, np_a, t_a), (res_b, par_b, np_b, t_b) = runs
        assert res_a == res_b and res_a[0] > 0 and np_a == np_b and t_a == t_b
        for k in par_a:
            assert torch.equal(par_a[k], par_b[k]), k
    finally:
        np.random.set_state(state)


@pytest.mark.parametrize("mode,factors", [("uniform", False), ("popularity", True)])
def test_sub_epoch_consumes_the_selected_negatives(golden, tmp_path, mode, factors):
    """neg_pool=3N: the negatives the step consumed satisfy the tolerance check against the epoch-start
    factors, the pools are the reference sampler's P draws per row, and numpy's stream ends where that
    sampler leaves it. factors=False: the trainer computes the absent factors itself, once."""
    P, H = 3 * N_NEG, 2
    state = np.random.get_state()
    try:
        tr, ds, loader = _trainer(golden, tmp_path, factors=factors, ds_kw=dict(neg_sampling=mode),
                                  neg_pool=P, neg_hard=H)
        assert (tr.user_factors is not None) == factors
        seen = []
        tr._on_negatives = lambda s, users, pool, negs, hard: seen.append(
            (s, users.clone(), pool.clone(), negs.clone(), hard.clone(), negs))
        start = np.random.get_state()
        n, loss = tr._train_epoch(loader)
        torch.cuda.synchronize()
        np_next = int(np.random.randint(0, 2 ** 31))
        assert n == 8 * len(seen) and len(seen) >= 3 and np.isfinite(loss) and loss > 0
        assert [s for s, *_ in seen] == list(range(len(seen)))
        assert len({c[5].data_ptr() for c in seen}) == 3  # the three negs buffers the steps read
        uf = tr.user_factors.cpu().numpy()        # the snapshot: not recomputed inside the sub-epoch
        itf = tr._item_feat_by_index().cpu().numpy()
        assert uf.shape == (tr.n_users, 32) and itf.shape[1] == 32

        neg = tr._negatives(ds)
        split, indptr, ranks = neg.split.cpu().numpy(), neg.indptr.cpu().numpy(), neg.ranks.cpu().numpy()
        w = np.ones(len(split), dtype=np.int64) if mode == "uniform" else ds.negative_weights()
        assert (neg.tables is not None) == (mode == "popularity")
        rs = np.random.RandomState()
        rs.set_state(start)
        n_hard = 0
        for _, users, pool, negs, hard, _ in seen:
            users, pool = users.cpu().numpy(), pool.cpu().numpy()
            want_pool = np.stack([WR.sample(rs, split, w, ranks[indptr[u]:indptr[u + 1]], P) for u in users])
            assert np.array_equal(pool, want_pool)
            R.check_against(uf, itf, users, pool, N_NEG, H, negs.cpu().numpy(), hard.cpu().numpy())
            n_hard += int(hard.sum())
        assert 0 < n_hard <= H * n
        assert np_next == int(rs.randint(0, 2 ** 31))
    finally:
        np.random.set_state(state)


def test_eval_loss_does_not_depend_on_neg_pool(golden, tmp_path):
    state = np.random.get_state()
    try:
        losses = []
        for kw in ({}, dict(neg_pool=3 * N_NEG)):
            tr, ds, _ = _trainer(golden, tmp_path, **kw)
            np.random.seed(5)
            torch.manual_seed(5)
            losses.append((tr._eval_epoch(ds), int(np.random.randint(0, 2 ** 31))))
        assert losses[0] == losses[1] and losses[0][0][0] == len(ds)
    finally:
        np.random.set_state(state)


def test_factors_of_another_dataset_raise_at_epoch_end(golden, tmp_path):
    """An item table shorter than the dataset's index space: the ids past it are out of range, never
    address it, and the sub-epoch ends in RuntimeError. The plain mode never looks at the factors."""
    state = np.random.get_state()
    try:
        tr, ds, loader = _trainer(golden, tmp_path, neg_pool=3 * N_NEG)
        whole = tr._item_feat_by_index
        tr._item_feat_by_index = lambda: whole()[:5].contiguous()
        with pytest.raises(RuntimeError, match="outside the factor tables"):
            tr._train_epoch(loader)
        torch.cuda.synchronize()
        tr, ds, loader = _trainer(golden, tmp_path, neg_pool=3 * N_NEG)
        tr.user_factors = tr.user_factors[:1].contiguous()  # and a user table that is too short
        with pytest.raises(RuntimeError, match="outside the factor tables"):
            tr._train_epoch(loader)
        torch.cuda.synchronize()
    finally:
        np.random.set_state(state)


def test_nonfinite_factors_warn(golden, tmp_path):
    state = np.random.get_state()
    try:
        tr, ds, loader = _trainer(golden, tmp_path, neg_pool=3 * N_NEG)
        tr.item_factors[:] = float("nan")
        with pytest.warns(RuntimeWarning, match="NaN or infinite"):
            n, loss = tr._train_epoch(loader)
        assert n > 0 and np.isfinite(loss)  # NaN factors choose nothing: the plain draws, a finite step
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="hard negatives")
            tr2, _, loader2 = _trainer(golden, tmp_path, neg_pool=3 * N_NEG)
            tr2._train_epoch(loader2)
    finally:
        np.random.set_state(state)


def test_checkpoint_carries_the_mode(golden, tmp_path):
    from dcrecommend.nn.dcue import DCUE
    tr, ds, _ = _trainer(golden, tmp_path, neg_pool=7, neg_hard=2)
    tr.save(models_dir=str(tmp_path))
    back = DCUE(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=N_NEG, lr=1e-3, device=DEV)
    back.load(os.path.join(str(tmp_path), tr._format_model_subdir()), tr.nn_epoch)
    assert (back.neg_pool, back.neg_hard) == (7, 2)
