"""Random-crop training over full-length tracks: DCUE(crop='epoch'), the multi-crop item factors and
embed_audio(crops=) against tests/crop_reference.py and host-cropped twins. Everything here is a copy
followed by kernels that exist already, so every comparison is bit for bit.

Shapes: tests/golden/eval.npz's 30 users x 48 songs (the trainer tests' dataset) and the plan shapes of
tests/test_gpu_plan.py (B = 8, N = 3, d = H = 32)."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

import crop_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return x.view(np.int16 if x.dtype == np.float16 else np.int64 if x.dtype == np.int64 else np.int32)


def _datasets(g, tmp_path, specs):
    """train / val / item sets over eval.npz's triplets with metadata row k pointing at specs[k] ([128, T])."""
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    from dcrecommend.datasets.dcuepredset import DCUEPredset
    os.makedirs(str(tmp_path), exist_ok=True)
    trip = pd.DataFrame({"user_id": g["raw_users"], "song_id": g["raw_songs"], "score": g["raw_score"]})
    paths = []
    for k, spec in enumerate(specs):
        p = os.path.join(str(tmp_path), "m%03d.pt" % k)
        if not os.path.exists(p):
            torch.save(torch.from_numpy(np.ascontiguousarray(spec, dtype=np.float32)), p)
        paths.append(p)
    meta = pd.DataFrame({"idx": np.arange(len(specs)), "song_id": g["meta_songs"], "data_mel": paths})
    return (DCUEPredset(trip.copy(), meta, split="train"), DCUEPredset(trip.copy(), meta, split="val"),
            DCUEItemset(trip.copy(), meta))


def _short_specs(g):
    """Every track at most 131 frames; three shorter ones, so the zero tail is part of the comparison."""
    specs = [np.array(s, dtype=np.float32) for s in g["spec"]]
    for k, L in ((0, 1), (1, 100), (2, 130)):
        specs[k] = specs[k][:, :L]
    return specs


def _long_specs(g):
    """fp16-representable tracks of 131 to 400 frames (131, 132 and 400 among them)."""
    rs = np.random.RandomState(5)
    n = len(g["meta_songs"])
    lengths = np.concatenate([[131, 132, 400], rs.randint(131, 401, n - 3)])
    return [rs.randn(128, int(L)).astype(np.float16).astype(np.float32) for L in lengths]


def _host_store(items, specs):
    """The store as the header lays it out, built from the spectrogram files' contents alone: item i's
    frames [T][128] one after the other in item-index order."""
    parts, lengths = [], []
    for i in range(len(items.item_index)):
        k = items.songid2metaindex[items.itemindex2songid[i]]
        parts.append(specs[k].T)
        lengths.append(specs[k].shape[1])
    return (np.ascontiguousarray(np.concatenate(parts), dtype=np.float16),
            np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))


def _trainer(train, crop, seed=7, **kw):
    from dcrecommend.nn.dcue import DCUE
    tr = DCUE(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=3, lr=1e-3, device=DEV, crop=crop, **kw)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    torch.manual_seed(seed)
    tr._init_nn()
    return tr


def _tower(tr, table):
    """dcue_item_tower_eval over a whole table, called directly: [n, d]."""
    from dcrecommend import _native as nat
    n = table.shape[0]
    dims = tr.model._flat["dims"]
    feat = torch.empty((n, nat.storage_dims(dims).feature_dim), device=DEV)
    ws = torch.empty(nat.workspace_bytes(dims, 1, 0, n), dtype=torch.uint8, device=DEV)
    it = torch.arange(n, dtype=torch.int32, device=DEV)
    tracks = nat.Tracks(table.data_ptr(), n, 0 if table.dtype == torch.float16 else 1, 0)
    model = tr.model._model_struct()
    tr.model.eval()
    nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(model), ctypes.byref(tracks), nat.ptr(it), n, nat.ptr(ws),
                                             ws.numel(), nat.ptr(feat), nat.stream_handle()), "dcue_item_tower_eval")
    return feat[:, :tr.feature_dim].clone()


@pytest.fixture(scope="module")
def long_case(golden, tmp_path_factory):
    g = golden("eval.npz")
    specs = _long_specs(g)
    train, val, items = _datasets(g, tmp_path_factory.mktemp("long"), specs)
    data, fp = _host_store(items, specs)
    return g, specs, train, val, items, data, fp


# ------------------------------------------------------------------------------- short tracks
def test_short_tracks_epoch_crops_change_nothing(golden, tmp_path):
    """All tracks <= 131 frames: every window is the whole track, so one fit epoch with crop='epoch'
    leaves the parameters, the user table, the losses and the factors identical to crop='load', and the
    three real factor passes give what the repeat-mean of one pass gives today."""
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    specs = _short_specs(g)
    runs = []
    for crop in ("load", "epoch"):
        train, val, items = _datasets(g, tmp_path / "mel", specs)
        losses = []

        class Rec(DCUE):
            def _train_epoch(self, loader):
                out = DCUE._train_epoch(self, loader)
                losses.append(out)
                return out

        tr = Rec(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=4, num_epochs=1, eval_pct=1.0, lr=1e-3,
                 device=DEV, crop=crop, crop_seed=3)
        np.random.seed(3)
        torch.manual_seed(3)
        tr.fit(train, val, val, val, train, items, len(train.user_index), len(train.item_index), "trip", "meta",
               str(tmp_path / ("ck_" + crop)))
        assert (tr._store is not None) == (crop == "epoch")
        state = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        fit_factors = tr.item_factors.clone()
        tr._item_factors(items, n_iter=3)
        runs.append((state, losses, fit_factors, tr.user_factors.clone(), tr.item_factors.clone(), tr._tracks.clone(),
                     tr.best_val_map))
    a, b = runs
    assert len(a[1]) == len(b[1]) >= 8 and a[1] == b[1]  # (samples, mean loss) of every train sub-epoch
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert "user_embd.embeddings.weight" in a[0]
    for i in (2, 3, 4, 5):
        assert np.array_equal(_bits(a[i]), _bits(b[i])), i
    assert a[6] == b[6] and float(a[4].abs().max()) > 0


# -------------------------------------------------------------------------------- long tracks
def test_track_store_and_recrop_equal_the_restatement(long_case):
    g, specs, train, val, items, data, fp = long_case
    dev_data, dev_fp = items.track_store(DEV)
    assert dev_data.dtype == torch.float16 and dev_fp.dtype == torch.int64
    assert np.array_equal(_bits(dev_data), _bits(data)) and np.array_equal(dev_fp.cpu().numpy(), fp)
    assert items.track_store(DEV, dtype=torch.float32)[0].dtype == torch.float32
    tr = _trainer(train, "epoch", crop_seed=9)
    tr._bind_items(items)
    ptr = tr._tracks.data_ptr()
    assert tr._tracks.shape == (len(items.item_index), 131, 128) and tr._tracks.dtype == torch.float16
    seen = []
    for e in (0, 1, 5):
        tr.nn_epoch = e
        flags = tr._recrop()
        assert not flags.any() and tr._tracks.data_ptr() == ptr
        want, starts, _ = R.crop(data, fp, None, np.float16, R.RANDOM, seed=9, draw=e)
        assert np.array_equal(_bits(tr._tracks), _bits(want)), e
        seen.append(starts)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # an explicit draw, and another seed
    tr._recrop(draw=1)
    assert np.array_equal(_bits(tr._tracks), _bits(R.crop(data, fp, None, np.float16, R.RANDOM, seed=9, draw=1)[0]))


def _plan_state(tr, plan):
    plan.sync()
    torch.cuda.synchronize()
    out = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    for k, v in tr.optimizer._adam_state().items():
        if k in ("m", "v", "em", "ev"):
            out["adam." + k] = v.clone()
    out["grad"] = tr.model._flat["G"].clone()
    return out


def test_recrop_between_steps_equals_a_host_cropped_twin(long_case):
    """Two steps with lookahead, the re-crop, two more steps -- against a twin whose tables were cropped
    on the host to the same starts before its plans were built. Both start from the same state and see
    the same users, items and negatives (catalogue item lists, given). Side streams and the lookahead
    are delayed on the re-cropping side, so a re-crop that did not wait for them, or a lookahead that
    survived it, would show."""
    from dcrecommend import _native as nat
    g, specs, train, val, items, data, fp = long_case
    B, N = 8, 3
    n_items = len(items.item_index)
    gen = torch.Generator(device=DEV).manual_seed(17)
    users = [torch.randint(0, len(train.user_index), (B,), generator=gen, device=DEV) for _ in range(4)]
    lists = [torch.randint(0, n_items, (B * (1 + N),), generator=gen, device=DEV).to(torch.int32) for _ in range(4)]
    tables = [torch.from_numpy(R.crop(data, fp, None, np.float16, R.RANDOM, seed=4, draw=e)[0]).to(DEV) for e in (1, 2)]
    assert not torch.equal(tables[0], tables[1])

    a = _trainer(train, "epoch", crop_seed=4)
    a._bind_items(items)
    plan = a._train_plan(N)
    losses_a = []
    try:
        for site in ("lookahead", "wgrad_hi", "wgrad_2", "user_bwd"):
            nat.debug_delay(site, 2000)
        for e, (s0, s1) in ((1, (0, 1)), (2, (2, 3))):
            a.nn_epoch = e
            a._recrop()
            assert plan is a._train_plan(N)  # the plan stays bound
            assert plan.set_next(lists[s1])
            with pytest.raises(RuntimeError, match="lookahead"):  # announced: no re-crop now
                a._recrop()
            plan.step(users[s0], lists[s0])
            with pytest.raises(RuntimeError, match="lookahead"):  # prepared ahead from the old rows
                a._recrop()
            plan.step(users[s1], lists[s1])
            losses_a.append(plan.loss.clone())
    finally:
        nat.debug_clear_delays()
    state_a = _plan_state(a, plan)
    assert np.array_equal(_bits(a._tracks), _bits(tables[1]))

    b = _trainer(train, "load")
    b._item_meta = items.item_rows()
    losses_b = []
    for table, (s0, s1) in zip(tables, ((0, 1), (2, 3))):
        b._tracks, b._plan = table, None
        twin = b._train_plan(N)
        assert twin.set_next(lists[s1])
        twin.step(users[s0], lists[s0])
        twin.step(users[s1], lists[s1])
        losses_b.append(twin.loss.clone())
        twin.sync()
        torch.cuda.synchronize()
        if table is tables[0]:
            twin.close()
    state_b = _plan_state(b, twin)
    for la, lb in zip(losses_a, losses_b):
        assert np.array_equal(_bits(la), _bits(lb)) and torch.isfinite(la)
    for k in state_a:
        assert torch.equal(state_a[k], state_b[k]), k
    # the announcement can be withdrawn; one more launch then leaves nothing prepared
    assert plan.set_next(lists[0])
    assert plan.set_next(None)
    a._recrop()
    plan.close()
    twin.close()


@pytest.mark.parametrize("factor_crops", ["random", "grid"])
def test_item_factors_average_real_passes(long_case, factor_crops):
    from dcrecommend import _native as nat
    g, specs, train, val, items, data, fp = long_case
    tr = _trainer(train, "epoch", crop_seed=6, factor_crops=factor_crops)
    tr._bind_items(items)
    before = tr._tracks.clone()
    tr._item_factors(items, n_iter=3)
    got = tr.item_factors
    assert torch.equal(tr._tracks, before)  # the training table is never touched
    meta = items.item_rows()
    rows = np.flatnonzero(meta >= 0).astype(np.int32)  # one chunk: fewer than 8,192 items
    acc = torch.zeros((len(rows), tr.feature_dim), device=DEV)
    passes = []
    for j in range(3):
        kw = dict(grid_j=j, grid_n=3) if factor_crops == "grid" else dict(seed=6, draw=R.FACTOR_DRAW0 + j)
        mode = R.GRID if factor_crops == "grid" else R.RANDOM
        table = torch.from_numpy(R.crop(data, fp, rows, np.float16, mode, **kw)[0]).to(DEV)
        passes.append(_tower(tr, table))
        acc += passes[-1]
    want = torch.zeros_like(got)
    want[torch.from_numpy(meta[rows]).to(DEV)] = acc / torch.tensor(3.0, device=DEV)
    assert np.array_equal(_bits(got), _bits(want))
    assert not torch.equal(passes[0], passes[1])  # the passes do differ: this is not the repeat-mean
    # get_item_factors goes the same way, and the factors are the same at every epoch
    tr.nn_epoch = 4
    assert np.array_equal(_bits(tr.get_item_factors(items, n_iter=3)), _bits(want))
    # one pass: the first random draw, or the grid's single window, the centre one
    first = passes[0] if factor_crops == "random" else _tower(
        tr, torch.from_numpy(R.crop(data, fp, rows, np.float16, R.CENTER)[0]).to(DEV))
    one = tr.get_item_factors(items, n_iter=1)
    assert np.array_equal(_bits(one[torch.from_numpy(meta[rows]).to(DEV)]), _bits(first))


def test_embed_audio_over_grid_windows(long_case):
    """crops=4 on equal-length clips of 3 x 131 frames: the fp32 mean, in order, of the four
    embed_audio(frame0=s_j) factors at the grid's starts -- the same launch shapes over the same input
    bits (a frame's log-mel row does not depend on the frame range it is computed in)."""
    g, specs, train, val, items, data, fp = long_case
    tr = _trainer(train, "load")
    rs = np.random.RandomState(2)
    T = 3 * 131
    x = (0.1 * rs.randn(3, (T - 1) * 512)).astype(np.float32)
    starts = [R.start(R.GRID, T, 0, grid_j=j, grid_n=4) for j in range(4)]
    assert starts == [0, 87, 174, 262]
    acc = torch.zeros((3, tr.feature_dim), device=DEV)
    for s in starts:
        acc += tr.embed_audio(x, frame0=s)
    want = acc / torch.tensor(4.0, device=DEV)
    got = tr.embed_audio(x, crops=4)
    assert got.shape == (3, tr.feature_dim) and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(tr.embed_audio(x, crops=1)), _bits(tr.embed_audio(x, frame0=(T - 131) // 2)))
    assert np.array_equal(_bits(tr.embed_audio(x[1], crops=4)), _bits(got[1:2]))  # one clip, 1-D
    assert not np.array_equal(_bits(got), _bits(tr.embed_audio(x)))
    with pytest.raises(ValueError, match="frame range"):
        tr.embed_audio(x[:, :66000], crops=2)  # 129 frames
    with pytest.raises(ValueError, match="crops"):
        tr.embed_audio(x, crops=0)
    with pytest.raises(ValueError, match="crops"):
        tr.embed_audio(x, frame0=3, crops=2)
    # the list calls pass it on
    tr._user_factors(items)
    tr._item_factors(items)
    tr.train_data = train
    q = tr.similar_to_audio(x, k=5, crops=4)
    assert [len(l) for l in q] == [5, 5, 5]
    assert [len(l) for l in tr.listeners_for_audio(x, k=4, crops=4)] == [4, 4, 4]


def test_checkpoint_keeps_the_crop_settings(long_case, tmp_path):
    from dcrecommend.nn.dcue import DCUE
    g, specs, train, val, items, data, fp = long_case
    tr = _trainer(train, "epoch", crop_seed=11, factor_crops="grid")
    tr.nn_epoch = 3
    tr.save(models_dir=str(tmp_path))
    sub = tmp_path / tr._format_model_subdir()
    ck = torch.load(str(sub / "epoch_3.pth"), weights_only=True)
    assert (ck["crop"], ck["crop_seed"], ck["factor_crops"]) == ("epoch", 11, "grid")
    tr2 = DCUE(device=DEV)
    tr2.load(str(sub), 3)
    assert (tr2.crop, tr2.crop_seed, tr2.factor_crops, tr2.nn_epoch) == ("epoch", 11, "grid", 4)
    # a resumed run continues the same sequence: the table bound after the load is draw nn_epoch's
    tr2._bind_items(items)
    assert np.array_equal(_bits(tr2._tracks), _bits(R.crop(data, fp, None, np.float16, R.RANDOM, seed=11, draw=4)[0]))
    # a checkpoint from before the crop settings loads as 'load', whatever the constructor said
    for k in ("crop", "crop_seed", "factor_crops"):
        del ck[k]
    torch.save(ck, str(sub / "epoch_2.pth"))
    tr3 = DCUE(device=DEV, crop="epoch", crop_seed=5, factor_crops="grid")
    tr3.load(str(sub), 2)
    assert (tr3.crop, tr3.crop_seed, tr3.factor_crops) == ("load", 0, "random") and tr3._store is None
    with pytest.raises(ValueError, match="crop"):
        DCUE(device=DEV, crop="batch")
    with pytest.raises(ValueError, match="factor_crops"):
        DCUE(device=DEV, factor_crops="centre")


def test_train_dcue_driver_crop_epoch(tmp_path):
    """train_dcue.py --crop epoch end to end on synthetic files: the options reach the trainer, the store
    is bound next to the table and the run trains and checkpoints as the default does."""
    import train_dcue
    dcue = train_dcue.main(["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80",
                            "--synthetic-pairs", "300", "--feature-dim", "32", "--conv-hidden", "32",
                            "--batch-size", "8", "--neg-batch-size", "3", "--num-epochs", "1",
                            "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path),
                            "--crop", "epoch", "--crop-seed", "2", "--factor-crops", "grid"])
    assert (dcue.crop, dcue.crop_seed, dcue.factor_crops) == ("epoch", 2, "grid")
    assert dcue._store is not None and dcue._store[1].numel() == dcue._tracks.shape[0] + 1
    assert dcue._plan_n == 3 and dcue.nn_epoch >= 9 and 0.0 <= dcue.best_val_auc <= 1.0
    assert os.listdir(tmp_path)
