"""GPU tests of the fold-in of unseen users (dcue_user_foldin / dcue_foldin_negatives, rank.FoldIn,
DCUE.fold_in / recommend_for, train_dcue.py --recommend-for) against the torch restatement in
foldin_reference.py: random towers built as DCUENet builds them, 600 to 2,500 Gaussian candidates, a
0.8 mask.

Tolerances are not constants: each comparison with the fp64 reference allows a multiple of the
reference's own fp32-vs-fp64 spread on the same case (8x for one step: the MFMA summation order;
50x for the loss after thirty steps: a near-tie may flip one step's active set), under the condition,
asserted on the case, that the fp64 reference has no (at most 0.1 % of its) hinge arguments within
1e-5 of zero.
"""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import foldin_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.int32)


def _on_gpu(c):
    """The case's net on the device, its dcue_model struct and a FoldIn over the case's mask."""
    from dcrecommend.nn import rank
    if "gpu" not in c:
        net = c["net"].to(DEV)
        net._require_device()
        c["gpu"] = (net, rank.FoldIn(c["mask"], DEV), torch.from_numpy(c["cand"]).to(DEV))
    return c["gpu"]


def _run(c, n_neg, steps, max_pos, margin=0.2, lr=0.05, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.0, seed=0,
         rows=None, user_batch=None, want_grad=True, init=None):
    """fold_in_raw over rows [rows[0], rows[1]) of the case (default: all), as numpy arrays."""
    from dcrecommend.nn import rank
    net, fi, cand = _on_gpu(c)
    lo, hi = rows if rows is not None else (0, len(c["hists"]))
    ptr, idx = R.csr(c["hists"])
    cfg = rank.FoldIn.config(steps, n_neg, max_pos, margin, lr, beta1, beta2, eps, weight_decay, seed)
    init = torch.from_numpy(c["init"][lo:hi] if init is None else init).to(DEV)
    out = fi.fold_in_raw(net._model_struct(), cand, ptr, idx, init, cfg, user_batch=user_batch, row0=lo,
                         want_grad=want_grad)
    return [None if t is None else t.cpu().numpy() for t in out]


# ------------------------------------------------------------------------------------- 1. sampler
@pytest.mark.parametrize("n_neg", [1, 5, 20])
def test_sampler_matches_the_python_restatement(n_neg):
    from dcrecommend.nn import rank
    c = R.make_case(40, 32, 600, R.ONE_STEP_LENS, 1)
    ok = np.flatnonzero(c["mask"])
    crowded = tuple(int(x) for x in ok if x not in (ok[3], ok[-7]))  # all but two eligible candidates
    hists = list(c["hists"]) + [crowded, ()]
    ptr, idx = R.csr(hists)
    fi = rank.FoldIn(c["mask"], DEV)
    max_pos = 16
    for seed in (0, 12345678901234567):
        cfg = rank.FoldIn.config(8, n_neg, max_pos, 0.2, 0.05, 0.9, 0.99, 1e-8, 0.0, seed)
        for step in (0, 7):
            for row0 in (0, 3):
                got = fi.negatives(ptr, idx, len(hists) - row0, cfg, step, row0=row0).cpu().numpy()
                want = np.stack([R.negatives(seed, r, step, hists[r], max_pos, n_neg, 600, c["mask"])
                                 for r in range(row0, len(hists))])
                assert np.array_equal(got, want), (seed, step, row0)
    r = len(hists) - 2
    assert (want[r - 3][:16] == -1).any() and set(np.unique(want[r - 3])) <= {-1, int(ok[3]), int(ok[-7])}
    assert np.all(want[-1] == -1)  # the empty history


def test_rejected_slots_set_flag_bit_2():
    c = dict(R.make_case(40, 32, 600, R.ONE_STEP_LENS, 1))
    ok = np.flatnonzero(c["mask"])
    crowded = tuple(int(x) for x in ok if x not in (ok[3], ok[-7]))
    c["hists"] = c["hists"][:2] + (crowded, ())
    c["init"] = c["init"][:4]
    c.pop("_ref", None)
    emb, feat, loss, grad, flags = _run(c, 5, 2, 16)
    ref = R.fold_in(c["weights"], c["cand"], c["mask"], c["hists"], c["init"], 2, 5, 16, 0.2, 0.05)
    assert flags.tolist() == ref["flags"].tolist() == [0, 0, R.DROPPED, R.EMPTY]
    # the empty history: row untouched, losses 0, its factor the tower of the initial row
    assert np.array_equal(_bits(emb[3]), _bits(c["init"][3])) and np.all(loss[3] == 0) and np.all(grad[3] == 0)
    np.testing.assert_allclose(feat[3], ref["feat"][3], rtol=0, atol=1e-5 * np.abs(ref["feat"][3]).max())
    np.testing.assert_allclose(loss, ref["loss"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------- 2. one step
@pytest.mark.parametrize("case", R.ONE_STEP_CASES)
def test_one_step_loss_and_gradient(case):
    """out_loss and out_grad of one step against the fp64 reference, within 8x the reference's own
    fp32-vs-fp64 spread on the same case (the gradient relative to its row's largest |g|). The
    spread is measured where the test runs; on the MI355X host it was (loss / gradient) E=40: d=32
    2.0e-7 / 3.0e-7, d=100 2.7e-8 / 2.3e-7, d=128 3.8e-7 / 3.1e-7, d=256 1.4e-7 / 4.5e-7; E=300: d=32
    1.8e-7 / 4.3e-7, d=100 2.9e-8 / 5.3e-7, d=128 3.0e-7 / 5.0e-7, d=256 1.0e-7 / 5.8e-7 -- so the
    tolerances used were 2.1e-7 .. 3.1e-6 on the loss and 1.8e-6 .. 4.7e-6 on the gradient, and the
    kernel's errors 4.3e-8 .. 8.4e-7 and 4.3e-7 .. 1.0e-6 (at most 4.0x and 3.1x the spread)."""
    E, d, n_cand, n_neg, seed = case
    c = R.make_case(E, d, n_cand, R.ONE_STEP_LENS, seed)
    r64 = R.reference(c, torch.float64, n_neg=n_neg, **R.ONE_STEP_CFG)
    r32 = R.reference(c, torch.float32, n_neg=n_neg, **R.ONE_STEP_CFG)
    assert r64["hinge"].size > 0 and not (np.abs(r64["hinge"]) < R.NEAR_TIE).any()
    sl, sg = R.spread(r32, r64)
    emb, feat, loss, grad, flags = _run(c, n_neg, **R.ONE_STEP_CFG)
    gmax = np.abs(r64["grad"]).max(axis=1)
    el = float(np.abs(loss.astype(np.float64) - r64["loss"]).max())
    eg = float((np.abs(grad.astype(np.float64) - r64["grad"]).max(axis=1) / gmax).max())
    print("one step %s: loss error %.3e (spread %.3e), gradient error %.3e (spread %.3e)" % (case, el, sl, eg, sg))
    assert flags.tolist() == r64["flags"].tolist()
    assert el <= 8 * sl, (el, sl)
    assert eg <= 8 * sg, (eg, sg)


@pytest.mark.parametrize("case", R.TIER_CASES)
def test_one_step_with_workspace_resident_rows(case):
    """The same rule where m and v (512, 673) or every activation (801, 1024) live in the workspace,
    and where E is no multiple of 4 (401, 673, 801). Measured on the MI355X host (loss / gradient):
    spreads 8.7e-8 .. 2.7e-7 / 5.8e-7 .. 8.1e-7, the kernel's errors 2.0e-7 .. 4.2e-7 / 5.3e-7 .. 9.9e-7
    (at most 4.4x and 1.4x the spread)."""
    test_one_step_loss_and_gradient(case)


# ------------------------------------------------------------------------------------- 3. Adam
@pytest.mark.parametrize("beta1", [0.9, 0.0])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-3])
@pytest.mark.parametrize("E,d", [(40, 32), (300, 100), (673, 32)])
def test_adam_step_is_the_trainers_bit_for_bit(E, d, weight_decay, beta1):
    """Given the gradient the kernel itself produced, the row after the step equals
    oracle.optim_oracle.adam_elementwise; the second step (moments and step count 2) too."""
    from oracle.optim_oracle import adam_elementwise
    c = R.make_case(E, d, 600, R.ONE_STEP_LENS, 1)
    kw = dict(max_pos=64, lr=0.05, beta1=beta1, beta2=0.99, eps=1e-8, weight_decay=weight_decay)
    emb1, _, _, grad1, _ = _run(c, 5, steps=1, **kw)
    zero = np.zeros_like(c["init"])
    p1, m1, v1 = adam_elementwise(c["init"], grad1, zero, zero, 0.05, beta1, 0.99, 1e-8, weight_decay, 1)
    assert np.abs(grad1).max() > 0
    assert np.array_equal(_bits(emb1), _bits(p1))
    emb2, _, _, grad2, _ = _run(c, 5, steps=2, **kw)
    p2, _, _ = adam_elementwise(p1, grad2, m1, v1, 0.05, beta1, 0.99, 1e-8, weight_decay, 2)
    assert np.array_equal(_bits(emb2), _bits(p2))


# ------------------------------------------------------------------------------------- 4. thirty steps
@pytest.mark.parametrize("case", R.THIRTY_CASES)
def test_thirty_steps(case):
    """Per-user final loss against fp64 within 50x the reference's fp32-vs-fp64 spread of it
    (measured on the MI355X host: 1.1e-7 at E = 40, d = 32 and 6.3e-8 at E = 300, d = 128, so 5.6e-6 and
    3.2e-6; the kernel's errors were 1.3e-7 and 8.4e-8)."""
    E, d, n_cand, n_neg, seed = case
    c = R.make_case(E, d, n_cand, R.THIRTY_LENS, seed)
    r64 = R.reference(c, torch.float64, n_neg=n_neg, **R.THIRTY_CFG)
    r32 = R.reference(c, torch.float32, n_neg=n_neg, **R.THIRTY_CFG)
    near = int((np.abs(r64["hinge"]) < R.NEAR_TIE).sum())
    assert near <= r64["hinge"].size // 1000, (near, r64["hinge"].size)
    sl = float(np.abs(r32["loss"][:, -1].astype(np.float64) - r64["loss"][:, -1]).max())
    emb, feat, loss, grad, flags = _run(c, n_neg, **R.THIRTY_CFG)
    el = float(np.abs(loss[:, -1].astype(np.float64) - r64["loss"][:, -1]).max())
    print("thirty steps %s: final loss error %.3e (spread %.3e); rows: error %.3e" %
          (case, el, sl, float(np.abs(emb - r64["emb"]).max())))
    assert el <= 50 * sl, (el, sl)
    assert loss[:, -1].mean() < loss[:, 0].mean()
    assert flags.tolist() == r64["flags"].tolist()


# ------------------------------------------------------------------------------------- 5. tiling
@pytest.mark.parametrize("E,d", [(40, 32), (300, 100), (512, 64), (801, 32)])
def test_tiling_and_batching_are_bit_identical(E, d):
    lens = tuple(int(x) for x in np.random.RandomState(4).randint(1, 41, 37))
    c = R.make_case(E, d, 900, lens, 3)
    kw = dict(n_neg=5, steps=5, max_pos=16)
    whole = _run(c, **kw)
    again = _run(c, **kw)
    chunks = _run(c, user_batch=16, **kw)  # 16, 16 and 5 users, each with its row0
    for a, b, e in zip(whole, again, chunks):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(e))
    assert np.isfinite(whole[2]).all() and (whole[2][:, -1] < whole[2][:, 0]).mean() > 0.5
    for n in (1, 16, 17):
        part = _run(c, rows=(0, n), **kw)
        for a, b in zip(whole, part):
            assert np.array_equal(_bits(a[:n]), _bits(b)), n
    tail = _run(c, rows=(32, 37), **kw)  # the third chunk on its own: row0 = 32
    for a, b in zip(whole, tail):
        assert np.array_equal(_bits(a[32:]), _bits(b))


# ------------------------------------------------------------------------------------- 6. steps = 0
@pytest.mark.parametrize("E,d", [(40, 32), (300, 100), (300, 256)])
def test_zero_steps_is_the_user_tower(E, d):
    """out_feat of a table row against dcue_user_tower's: the fold-in GEMMs sum k in another order
    than tgemm_block, so (E + 8) 2^-24 relative to the row's largest entry."""
    c = R.make_case(E, d, 600, R.ONE_STEP_LENS, 1)
    net, _, _ = _on_gpu(c)
    table = net.user_embd.embeddings.weight.detach()
    rows = np.array([0, 1, 2, 3, 1, 0])
    init = table[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    emb, feat, loss, grad, flags = _run(c, 5, steps=0, max_pos=64, init=init, want_grad=False)
    want = net.user_features(torch.from_numpy(rows).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(emb), _bits(init)) and loss.shape == (6, 0) and not flags.any()
    err = np.abs(feat - want).max(axis=1) / np.abs(want).max(axis=1)
    print("steps = 0, E = %d, d = %d: relative error %.3e (bound %.3e)" % (E, d, err.max(), (E + 8) * 2.0 ** -24))
    assert np.all(err <= (E + 8) * 2.0 ** -24)


# ------------------------------------------------------------------------------------- 7. frozen model
def _train_step(net, opt, u, pos, neg):
    net.train()
    opt.zero_grad()
    scores = net(u, pos, neg)[0]
    torch.max(torch.zeros_like(scores), 0.2 - scores).sum(dim=1).mean().backward()
    opt.step()
    torch.cuda.synchronize()


def _state(net, opt):
    st = opt._adam_state()
    fl = net._flat
    return [t.detach().clone() for t in (fl["P"], net.user_embd.embeddings.weight, st["m"], st["v"], st["em"], st["ev"],
                                         fl["stats"], fl["nbt"])]


def test_model_is_frozen():
    from dcrecommend.dcue.dcue import DCUENet
    from dcrecommend.nn import rank
    from dcrecommend.optim import NativeAdam
    gen = torch.Generator().manual_seed(3)
    u = torch.randint(0, 6, (3,), generator=gen).to(DEV)
    pos = torch.randn(3, 128, 131, generator=gen).half().float().to(DEV)
    neg = torch.randn(3, 2, 128, 131, generator=gen).half().float().to(DEV)
    c = R.make_case(40, 32, 600, R.ONE_STEP_LENS, 1)
    ptr, idx = R.csr(c["hists"])
    states = []
    for fold in (True, False):
        torch.manual_seed(11)
        net = DCUENet({"feature_dim": 32, "conv_hidden": 32, "user_embdim": 40, "user_count": 6,
                       "model_type": "truedcuemel1dbn"}).to(DEV)
        opt = NativeAdam(net.parameters(), 1e-3, (0.9, 0.99), 1e-8, 0)
        _train_step(net, opt, u, pos, neg)
        if fold:
            before = _state(net, opt)
            fi = rank.FoldIn(c["mask"], DEV)
            cfg = rank.FoldIn.config(5, 5, 16, 0.2, 0.05, 0.9, 0.99, 1e-8)
            out = fi.fold_in_raw(net._model_struct(opt._adam_state()), torch.from_numpy(c["cand"]).to(DEV), ptr, idx,
                                 torch.from_numpy(c["init"]).to(DEV), cfg)
            assert float(out[2][:, -1].mean()) < float(out[2][:, 0].mean())
            for a, b in zip(before, _state(net, opt)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        _train_step(net, opt, u, pos, neg)
        states.append(_state(net, opt))
    for a, b in zip(*states):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------- 8. API
def _datasets(g, tmp_path):
    from dcrecommend.datasets.dcuepredset import DCUEPredset
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    trip = pd.DataFrame({"user_id": g["raw_users"], "song_id": g["raw_songs"], "score": g["raw_score"]})
    paths = []
    for k in range(len(g["meta_songs"])):
        p = os.path.join(str(tmp_path), "m%03d.pt" % k)
        torch.save(torch.from_numpy(g["spec"][k].astype(np.float32)), p)
        paths.append(p)
    meta = pd.DataFrame({"idx": np.arange(len(g["meta_songs"])), "song_id": g["meta_songs"], "data_mel": paths})
    return (DCUEPredset(trip.copy(), meta, split="train"), DCUEPredset(trip.copy(), meta, split="val"),
            DCUEItemset(trip.copy(), meta))


@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    train, val, items = _datasets(g, tmp_path_factory.mktemp("mel"))
    tr = DCUE(feature_dim=int(g["d"]), conv_hidden=int(g["H"]), batch_size=8, device=DEV, lr=0.05)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    tr._init_nn()
    tr.model.load_state_dict({k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd.")})
    with pytest.raises(RuntimeError, match="no factors"):
        tr.fold_in([[g["val_songs"][0]]])
    with pytest.raises(RuntimeError, match="no factors"):
        tr.recommend_for([[g["val_songs"][0]]])
    tr._user_factors(items)
    tr._item_factors(items)
    tr.train_data = train
    return g, tr, train, val, items


def test_recommend_for_is_fold_in_then_topk(trained):
    from dcrecommend.nn import rank
    g, tr, train, val, items = trained
    with_audio = [train.itemindex2songid[int(i)] for i in np.flatnonzero(tr._item_meta >= 0)]
    rs = np.random.RandomState(2)
    histories = [list(rs.choice(with_audio, n, replace=False)) for n in (1, 3, 8, 20)]
    feat = tr.fold_in(histories, steps=10, n_neg=4, seed=5)
    assert feat.shape == (4, tr.feature_dim) and feat.is_cuda and bool(torch.isfinite(feat).all())
    assert torch.equal(feat, tr.fold_in(histories, steps=10, n_neg=4, seed=5))
    assert not torch.equal(feat, tr.fold_in(histories, steps=10, n_neg=4, seed=6))
    idx, score, count = tr.recommend_for(histories, k=7, as_ids=False, steps=10, n_neg=4, seed=5)
    played = [sorted(train.item_index[s] for s in h) for h in histories]
    ptr, excl = R.csr(played)
    want = rank.TopK(ptr, excl, (tr._item_meta >= 0).astype(np.uint8), DEV).topk(
        feat, tr._item_feat_by_index(), np.arange(4), 7)
    assert np.array_equal(idx, want[0]) and np.array_equal(_bits(score), _bits(want[1])) and np.array_equal(count, want[2])
    for r in range(4):
        assert count[r] == 7 and not np.isin(idx[r], played[r]).any()
    pairs = tr.recommend_for(histories, k=7, steps=10, n_neg=4, seed=5)
    assert [[s for s, _ in lst] for lst in pairs] == [[train.itemindex2songid[int(i)] for i in row] for row in idx]
    # the history allowed back in: the user's own songs may now be listed
    idx2 = tr.recommend_for(histories, k=7, as_ids=False, exclude_history=False, steps=10, n_neg=4, seed=5)[0]
    assert idx2.shape == (4, 7)
    # a split's candidates only
    for lst in tr.recommend_for(histories[:2], k=3, dataset=val, steps=5, n_neg=4):
        assert all(s in set(val.uniq_songs) for s, _ in lst)
    # the loss the fold-in minimises falls
    usable, _ = tr._history_items(histories, None)
    loss = tr._fold_in(usable, None, 10, 4, None, 64, 5, None)[2]
    assert float(loss[:, -1].mean()) < float(loss[:, 0].mean())


def test_fold_in_errors(trained):
    g, tr, train, val, items = trained
    song = g["val_songs"][0]
    with pytest.raises(KeyError):
        tr.fold_in([[song, "no such song"]])
    with pytest.raises(KeyError):
        tr.recommend_for([[song], ["no such song"]])
    with pytest.raises(TypeError):
        tr.recommend_for([[song]], stepz=3)
    with pytest.raises(ValueError):
        tr.fold_in([[song]], n_neg=0)
    # a history whose songs have no audio: nothing to fold in from
    meta = tr._item_meta
    i = train.item_index[song]
    tr._item_meta = meta.copy()
    tr._item_meta[i] = -1
    try:
        with pytest.raises(ValueError, match="no song with audio"):
            tr.fold_in([[song]])
        other = next(s for s in g["val_songs"] if train.item_index[s] != i and meta[train.item_index[s]] >= 0)
        lst = tr.recommend_for([[song, other]], k=5, steps=3, n_neg=3)[0]  # dropped from the positives,
        assert song not in [s for s, _ in lst] and other not in [s for s, _ in lst]  # kept in the exclusion list
    finally:
        tr._item_meta = meta
        tr._evals = {k: v for k, v in tr._evals.items() if k[0] != "foldin"}


def test_train_dcue_driver_recommends_for_new_users(tmp_path):
    import train_dcue
    mel = tmp_path / "mel"
    mel.mkdir()
    trip, _ = train_dcue.synthetic_data(24, 80, 300, str(mel), 0)  # the ids the driver will train on
    songs = sorted(set(trip["song_id"]))
    rs = np.random.RandomState(1)
    new = {"n%02d" % u: list(rs.choice(songs, 3 + u, replace=False)) for u in range(5)}
    src = tmp_path / "new.csv"
    pd.DataFrame([(u, s) for u, h in new.items() for s in h], columns=["user_id", "song_id"]).to_csv(src, index=False)
    out = tmp_path / "rec.csv"
    argv = ["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80", "--synthetic-pairs", "300",
            "--feature-dim", "32", "--conv-hidden", "32", "--batch-size", "8", "--neg-batch-size", "3",
            "--num-epochs", "1", "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path / "ck"),
            "--recommend-k", "5", "--recommend-out", str(out), "--recommend-for", str(src)]
    train_dcue.main(argv)
    rec = pd.read_csv(out)
    assert list(rec.columns) == ["user_id", "rank", "song_id", "score"]
    assert list(dict.fromkeys(rec["user_id"])) == list(new)
    for u, grp in rec.groupby("user_id"):
        assert grp["rank"].tolist() == [1, 2, 3, 4, 5]
        assert grp["score"].tolist() == sorted(grp["score"], reverse=True)
        assert len(set(grp["song_id"])) == 5 and not set(grp["song_id"]) & set(new[u])
        assert set(grp["song_id"]) <= set(songs)
