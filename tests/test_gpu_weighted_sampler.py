"""dcue_sample_catalogue_weighted and the trainer path over it against the definition in
weighted_sampler_reference.py (numpy's legacy randint + cumsum + searchsorted). Integers only: every
comparison is exact, outputs and stream positions.

Shape: test_catalogue_sampler_groups_and_long_lists' (tests/test_gpu_parity.py): 12,000 songs, a
10,000-song split, 300 users, 700 samples (several groups of the stream kernel), one user with more
than 8,192 split items (searched in global memory), one with a single candidate of weight 1
(W_u == 1: no draw), one with no positive-weight candidate (W_u == 0: a row of -1, no draw), users
with no split items, 20 % zero weights."""
import ctypes
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import weighted_sampler_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXW = 2 ** 32 - 1
U_LONG, U_ONE, U_NONE_LEFT, U_EMPTY = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(split, w, indptr, ranks, users_seq, next users); kind: 'small' weights below 200, 'large' the
    same scaled to a total in (2^31, 2^32 - 1] (the rejection mask is all ones), 'unit' all ones."""
    from dcrecommend.datasets.csr import user_split_ranks
    rs = np.random.RandomState(5)
    n_songs, n_users, n = 12000, 300, 10000
    split = np.sort(rs.choice(n_songs, n, replace=False)).astype(np.int64)
    w = rs.randint(1, 200, n).astype(np.int64)
    w[rs.rand(n) < 0.2] = 0
    w[:3] = 0
    w[-3:] = 0
    if kind == "large":
        w *= MAXW // int(w.sum())
    one = int(np.nonzero(w)[0][1234])
    w[one] = 1
    if kind == "unit":
        w[:] = 1
    pos = np.nonzero(w)[0]
    pairs = [(U_LONG, int(x)) for x in rs.choice(split, 9000, replace=False)]  # > the 8192-entry stage
    if kind == "unit":
        pairs += [(U_ONE, int(x)) for x in split[1:]] + [(U_NONE_LEFT, int(x)) for x in split]
    else:
        pairs += [(U_ONE, int(split[p])) for p in pos if p != one] + [(U_NONE_LEFT, int(split[p])) for p in pos]
    for u in range(4, n_users):
        pairs += [(u, int(x)) for x in rs.choice(n_songs, rs.randint(0, 60), replace=False)]
    uidx = np.array([p[0] for p in pairs], dtype=np.int64)
    sidx = np.array([p[1] for p in pairs], dtype=np.int64)
    indptr, ranks = user_split_ranks(uidx, sidx, n_users, split)
    users_seq = rs.randint(4, n_users, 700).astype(np.int64)
    users_seq[[3, 100, 250, 251, 400, 600, 699]] = [U_LONG, U_EMPTY, U_ONE, U_LONG, U_NONE_LEFT, U_ONE, U_NONE_LEFT]
    nxt = rs.randint(3, n_users, 50).astype(np.int64)
    if kind == "large":
        assert 2 ** 31 < int(w.sum()) <= MAXW
    return split, w, indptr, ranks, users_seq, nxt


@functools.lru_cache(maxsize=None)
def _want(kind, N, reseed):
    """The definition over users_seq + the next users (one stream), computed once and left unchanged."""
    split, w, indptr, ranks, users_seq, nxt = _case(kind)
    state = np.random.get_state()
    try:
        out = R.sample_users(1234 if reseed else 77, reseed, split, w, indptr, ranks, np.concatenate([users_seq, nxt]), N)
    finally:
        np.random.set_state(state)
    out.setflags(write=False)
    return out


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


class _Device:
    """The case's arrays on the device and the dcue_weight_tables over them."""

    def __init__(self, kind):
        from dcrecommend import _native as nat
        from dcrecommend.datasets.csr import weighted_split_tables
        split, w, indptr, ranks, _, _ = _case(kind)
        self.split, self.indptr, self.ranks = _dev(split, torch.int64), _dev(indptr, torch.int64), _dev(ranks, torch.int32)
        self.host = weighted_split_tables(indptr, ranks, w)
        self.arrays = [torch.from_numpy(a.view(np.int32)).to(DEV) for a in self.host]  # uint32 bits
        self.tables = nat.WeightTables(*[a.data_ptr() for a in self.arrays])

    def weighted(self, state, reseed, seed, users, N):
        from dcrecommend import _native as nat
        us = _dev(users, torch.int64)
        out = torch.full((len(users), N), -7, dtype=torch.int64, device=DEV)
        nat.check(nat.lib().dcue_sample_catalogue_weighted(
            None if state is None else nat.ptr(state), reseed, seed, nat.ptr(self.split), self.split.numel(),
            nat.ptr(self.indptr), nat.ptr(self.ranks), ctypes.byref(self.tables), nat.ptr(us), us.numel(), N,
            nat.ptr(out), nat.stream_handle()), "dcue_sample_catalogue_weighted")
        return out.cpu().numpy()

    def uniform(self, state, reseed, seed, users, N):
        from dcrecommend import _native as nat
        us = _dev(users, torch.int64)
        out = torch.full((len(users), N), -7, dtype=torch.int64, device=DEV)
        nat.check(nat.lib().dcue_sample_catalogue(
            None if state is None else nat.ptr(state), reseed, seed, nat.ptr(self.split), self.split.numel(),
            nat.ptr(self.indptr), nat.ptr(self.ranks), nat.ptr(us), us.numel(), N, nat.ptr(out),
            nat.stream_handle()), "dcue_sample_catalogue")
        return out.cpu().numpy()


def _mt_state(seed):
    from dcrecommend import _native as nat
    st = torch.zeros(nat.MT_STATE_BYTES, dtype=torch.uint8, device=DEV)  # the pad words are never written
    nat.check(nat.lib().dcue_mt_seed(nat.ptr(st), seed, nat.stream_handle()), "seed")
    return st


def _check_special_rows(kind, got, users):
    split, w, _, _, _, _ = _case(kind)
    assert (got[users == U_NONE_LEFT] == -1).all() and (got[users != U_NONE_LEFT] >= 0).all()
    one = got[users == U_ONE]
    assert len(one) and (one == one[0, 0]).all() and w[np.searchsorted(split, one[0, 0])] == 1
    assert not np.isin(got[users != U_NONE_LEFT], split[w == 0]).any()  # a zero-weight song is never drawn


@pytest.mark.parametrize("kind", ["small", "large"])
@pytest.mark.parametrize("N", [20, 1, 300])
def test_stream_equals_the_definition(kind, N):
    _, _, _, _, users_seq, nxt = _case(kind)
    want = _want(kind, N, False)
    d = _Device(kind)
    st = _mt_state(77)
    got = d.weighted(st, 0, 0, users_seq, N)
    assert np.array_equal(got, want[:len(users_seq)])
    _check_special_rows(kind, got, users_seq)
    # the stream continues where numpy's does: the next call equals the definition's next samples
    assert np.array_equal(d.weighted(st, 0, 0, nxt, N), want[len(users_seq):])


@pytest.mark.parametrize("kind", ["small", "large"])
@pytest.mark.parametrize("N", [20, 300])
def test_reseed_equals_the_definition(kind, N):
    _, _, _, _, users_seq, _ = _case(kind)
    want = _want(kind, N, True)[:len(users_seq)]
    d = _Device(kind)
    got = d.weighted(None, 1, 1234, users_seq, N)
    assert np.array_equal(got, want)
    _check_special_rows(kind, got, users_seq)


@pytest.mark.parametrize("N", [20, 1, 300])
def test_unit_weights_are_the_uniform_sampler(N):
    """w == 1 everywhere: dcue_sample_catalogue's outputs in both protocols, and its state afterwards."""
    _, _, _, _, users_seq, nxt = _case("unit")
    d = _Device("unit")
    assert int(d.host[3][U_ONE]) == 1 and int(d.host[3][U_NONE_LEFT]) == 0
    a, b = _mt_state(77), _mt_state(77)
    for users in (users_seq, nxt):
        assert np.array_equal(d.weighted(a, 0, 0, users, N), d.uniform(b, 0, 0, users, N))
        assert torch.equal(a, b)
    assert not torch.equal(a, _mt_state(77))
    assert np.array_equal(d.weighted(None, 1, 1234, users_seq, N), d.uniform(None, 1, 1234, users_seq, N))


def test_validation():
    from dcrecommend import _native as nat
    d = _Device("small")
    users = _dev(_case("small")[4][:4], torch.int64)
    out = torch.full((4, 20), -7, dtype=torch.int64, device=DEV)
    st = _mt_state(1)
    before = st.clone()
    torch.cuda.synchronize()
    OK, INVALID, UNSUPPORTED = 0, 1, nat.ERR_UNSUPPORTED

    def call(state=st, reseed=0, split=d.split, n_split=None, indptr=d.indptr, ranks=d.ranks, tables=d.tables,
             users=users, n_samples=4, N=20, out=out):
        return nat.lib().dcue_sample_catalogue_weighted(
            nat.ptr(state), reseed, 5, nat.ptr(split), d.split.numel() if n_split is None else n_split,
            nat.ptr(indptr), nat.ptr(ranks), None if tables is None else ctypes.byref(tables), nat.ptr(users),
            n_samples, N, nat.ptr(out), nat.stream_handle())

    launches = nat.lib().dcue_launch_count()
    assert call(tables=None) == INVALID
    for k in range(4):  # each table of the struct
        ptrs = [a.data_ptr() for a in d.arrays]
        ptrs[k] = None
        assert call(tables=nat.WeightTables(*ptrs)) == INVALID, k
    for name in ("split", "indptr", "ranks", "users", "out"):
        assert call(**{name: None}) == INVALID, name
    assert call(N=1025) == INVALID
    assert call(N=-1) == INVALID and call(n_samples=-1) == INVALID and call(n_split=-1) == INVALID
    assert call(state=None) == INVALID          # the global stream needs a state
    assert call(n_split=2 ** 31) == UNSUPPORTED  # stream form, as dcue_sample_catalogue
    assert call(n_samples=0) == OK and call(N=0) == OK
    assert call(state=None, reseed=1, n_samples=0) == OK
    assert nat.lib().dcue_launch_count() == launches
    torch.cuda.synchronize()
    assert (out == -7).all() and torch.equal(st, before)
    assert call(N=1024, out=torch.empty((4, 1024), dtype=torch.int64, device=DEV)) == OK
    assert call(state=None, reseed=1) == OK
    assert nat.lib().dcue_launch_count() == launches + 2
    torch.cuda.synchronize()
    assert (out >= 0).all()


# ------------------------------------------------------------------------------------- trainer
def _frames(g, tmp_path=None):
    """tests/golden/eval.npz's triplets (30 users x 48 songs, the golden fit's set) and metadata."""
    trip = pd.DataFrame({"user_id": g["raw_users"], "song_id": g["raw_songs"], "score": g["raw_score"]})
    paths = [""] * len(g["meta_songs"])
    if tmp_path is not None:
        for k in range(len(paths)):
            paths[k] = os.path.join(str(tmp_path), "m%03d.pt" % k)
            torch.save(torch.from_numpy(g["spec"][k].astype(np.float32)), paths[k])
    meta = pd.DataFrame({"idx": np.arange(len(paths)), "song_id": g["meta_songs"], "data_mel": paths})
    return trip, meta


def test_negatives_draw_equals_the_host_path(golden):
    """_Negatives.draw over three consecutive batches continues numpy's stream exactly as
    DCUEDataset._user_nonitem_songids called in the same order does, and hands it back there."""
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.nn.dcue import _Negatives, _mt_from_numpy, _mt_to_numpy
    trip, meta = _frames(golden("eval.npz"))
    state = np.random.get_state()
    try:
        ds = DCUEDataset(trip.copy(), meta, neg_samples=5, split="train", neg_sampling="popularity")
        assert len(set(ds.negative_weights().tolist())) > 3
        neg = _Negatives(ds, DEV)
        assert neg.tables is not None
        u_all, _ = ds.split_rows()
        rows = np.random.RandomState(2).permutation(len(u_all))[:24].reshape(3, 8)
        np.random.seed(31)
        want = [[[ds.item_index[s] for s in ds._user_nonitem_songids(ds.userindex2userid[int(u_all[r])])]
                 for r in batch] for batch in rows]
        host_next = np.random.randint(0, 2 ** 31, 5)
        np.random.seed(31)
        mt = _mt_from_numpy(DEV)
        np.random.seed(99)  # the device carries the stream now
        for batch, w in zip(rows, want):
            users = torch.from_numpy(u_all[batch]).to(DEV)
            out = torch.empty((8, 5), dtype=torch.int64, device=DEV)
            neg.check(users)
            neg.draw(mt, users, 5, out)
            assert out.cpu().numpy().tolist() == w
        _mt_to_numpy(mt)
        assert np.array_equal(np.random.randint(0, 2 ** 31, 5), host_next)
    finally:
        np.random.set_state(state)


def _sub_epoch(golden, tmp_path, **ds_kw):
    """One training sub-epoch of a fresh trainer over eval.npz's train split: (dataset, _Negatives,
    (samples, loss), parameters, the numpy draw after it)."""
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    from dcrecommend.nn.dcue import DCUE
    trip, meta = _frames(golden("eval.npz"), tmp_path)
    ds = DCUEDataset(trip.copy(), meta, neg_samples=3, split="train", **ds_kw)
    items = DCUEItemset(trip.copy(), meta)
    tr = DCUE(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=3, lr=1e-3, device=DEV)
    tr.n_users, tr.n_items, tr.epoch_size = len(ds.user_index), len(ds.item_index), 64
    tr.train_data = ds
    np.random.seed(13)
    torch.manual_seed(13)
    tr._init_nn()
    tr._bind_items(items)
    loader = tr._batch_loaders(ds, k=10)[0]
    tr.scheduler.step()
    res = tr._train_epoch(loader)
    torch.cuda.synchronize()
    params = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    return ds, tr._negatives(ds), res, params, int(np.random.randint(0, 2 ** 31))


def test_fit_sub_epoch_with_popularity_negatives(golden, tmp_path):
    state = np.random.get_state()
    try:
        ds, neg, (n, loss), params, _ = _sub_epoch(golden, tmp_path, neg_sampling="popularity", neg_alpha=0.75)
        assert neg.tables is not None and n > 0 and np.isfinite(loss) and loss > 0
        assert all(bool(torch.isfinite(v).all()) for v in params.values() if v.is_floating_point())
    finally:
        np.random.set_state(state)


def test_uniform_mode_is_unchanged(golden, tmp_path):
    """'uniform', spelled out or by default: the uniform entry point, the same negatives, loss bits,
    parameters and numpy stream."""
    from dcrecommend.nn.dcue import _mt_from_numpy
    state = np.random.get_state()
    try:
        runs = [_sub_epoch(golden, tmp_path), _sub_epoch(golden, tmp_path, neg_sampling="uniform", neg_alpha=0.3)]
        (ds_a, neg_a, res_a, par_a, nxt_a), (ds_b, neg_b, res_b, par_b, nxt_b) = runs
        assert ds_a.neg_sampling == ds_b.neg_sampling == "uniform"
        assert neg_a.tables is None and neg_b.tables is None
        assert res_a == res_b and res_a[0] > 0 and nxt_a == nxt_b
        for k in par_a:
            assert torch.equal(par_a[k], par_b[k]), k
        users = torch.from_numpy(ds_a.split_rows()[0][:16].copy()).to(DEV)
        outs = []
        for neg in (neg_a, neg_b):
            np.random.seed(4)
            mt = _mt_from_numpy(DEV)
            out = torch.empty((16, 3), dtype=torch.int64, device=DEV)
            neg.draw(mt, users, 3, out)
            outs.append((out.cpu(), mt.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        np.random.seed(4)  # and they are the reference's np.random.choice over the non-items
        want = [[ds_a.item_index[s] for s in ds_a._user_nonitem_songids(ds_a.userindex2userid[int(u)])] for u in users.cpu()]
        assert outs[0][0].numpy().tolist() == want
    finally:
        np.random.set_state(state)
