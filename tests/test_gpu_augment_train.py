"""DCUE(crop='epoch', augment=...): the training sub-epoch's table against tests/augment_reference.py, and
the clean-table rule -- validation losses, item factors and embed_audio never see a masked or gain-shifted
window. tests/test_gpu_crop_train.py's setting: eval.npz's 30 users x 48 songs, tracks of 131 to 400
frames, B = 8, N = 3, d = H = 32. Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import augment_reference as A
import crop_reference as R
import test_gpu_crop_train as T
from test_gpu_crop_train import long_case  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu
DEV = T.DEV
AUG = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=40, gain_db=6.0)
REF_AUG = A.Aug(2, 27, 2, 40, 6.0)


def _sub_epoch(tr, train, epoch, seed=3):
    """One training sub-epoch at nn_epoch = epoch, as fit runs it."""
    tr.nn_epoch = epoch
    tr.train_data = train
    np.random.seed(seed)
    torch.manual_seed(seed)
    loader = tr._batch_loaders(train, k=10)[0]
    tr.scheduler.step()
    out = tr._train_epoch(loader)
    torch.cuda.synchronize()
    return out


def _eval(tr, val, seed=5):
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = tr._eval_epoch(val)
    torch.cuda.synchronize()
    return out


def _count_recrops(tr):
    calls = []
    inner = tr._recrop

    def counted(*a, **kw):
        calls.append((a, kw))
        return inner(*a, **kw)

    tr._recrop = counted
    return calls


def test_train_table_is_augmented_and_evaluation_reads_the_clean_one(long_case):
    g, specs, train, val, items, data, fp = long_case
    state = np.random.get_state()
    try:
        tr = T._trainer(train, "epoch", crop_seed=9, augment=AUG)
        assert tr.augment == dict(fill="mean", **AUG)
        tr._bind_items(items)
        clean = {e: R.crop(data, fp, None, np.float16, R.RANDOM, seed=9, draw=e)[0] for e in (0, 1, 2)}
        masked = {e: A.crop(data, fp, None, np.float16, REF_AUG, seed=9, draw=e)[0] for e in (1, 2)}
        assert np.array_equal(T._bits(tr._tracks), T._bits(clean[0])) and not tr._tracks_dirty  # binding cuts clean
        n, loss = _sub_epoch(tr, train, 1)
        assert n > 0 and np.isfinite(loss)
        assert np.array_equal(T._bits(tr._tracks), T._bits(masked[1])) and tr._tracks_dirty
        assert not np.array_equal(T._bits(masked[1]), T._bits(clean[1]))

        # the evaluation first cuts the same windows again, clean -- once
        calls = _count_recrops(tr)
        loss_a = _eval(tr, val)
        assert len(calls) == 1 and not tr._tracks_dirty
        assert np.array_equal(T._bits(tr._tracks), T._bits(clean[1]))
        assert _eval(tr, val) == loss_a and len(calls) == 1  # a second evaluation re-cuts nothing
        del tr._recrop

        # a trainer with the same weights and no augment, at the same epoch
        twin = T._trainer(train, "epoch", crop_seed=9)
        assert twin.augment is None
        twin._bind_items(items)
        twin.model.load_state_dict(tr.model.state_dict())
        twin.nn_epoch = 1
        twin._recrop()
        loss_b = _eval(twin, val)
        assert loss_a == loss_b and np.isfinite(loss_a[1]) and loss_a[0] > 0

        # an evaluation that read the masked table would not have passed: its loss is another number
        tr._recrop(augment=True)
        assert np.array_equal(T._bits(tr._tracks), T._bits(masked[1]))
        tr._tracks_dirty = False  # as if nothing tracked it
        assert _eval(tr, val) != loss_a
        tr._tracks_dirty = True

        # the next sub-epoch: another table, from (crop_seed, nn_epoch) alone
        _sub_epoch(tr, train, 2)
        assert np.array_equal(T._bits(tr._tracks), T._bits(masked[2]))
        assert not np.array_equal(T._bits(masked[2]), T._bits(masked[1]))
        if tr._plan is not None:
            tr._plan.close()
    finally:
        np.random.set_state(state)


def test_factors_and_embed_audio_stay_clean(long_case):
    g, specs, train, val, items, data, fp = long_case
    state = np.random.get_state()
    try:
        outs = []
        for kw in (dict(augment=AUG), {}):
            tr = T._trainer(train, "epoch", crop_seed=6, **kw)
            tr._bind_items(items)
            if kw:  # with the masked table of a training re-crop in place
                tr.nn_epoch = 1
                tr._recrop(augment=True)
                assert tr._tracks_dirty
                before = tr._tracks.clone()
            tr._item_factors(items, n_iter=3)
            if kw:
                assert torch.equal(tr._tracks, before)  # the factor passes cut into their own scratch table
            rs = np.random.RandomState(2)
            x = (0.1 * rs.randn(2, (3 * 131 - 1) * 512)).astype(np.float32)
            outs.append((tr.item_factors.clone(), tr.embed_audio(x, crops=3).clone()))
        for a, b in zip(*outs):
            assert np.array_equal(T._bits(a), T._bits(b)) and float(a.abs().max()) > 0
    finally:
        np.random.set_state(state)


def test_no_augment_is_the_trainer_as_it_was(long_case):
    """augment=None, spelled out or by default: the same sub-epoch -- loss, parameters, table, numpy stream."""
    from dcrecommend.nn.dcue import DCUE
    g, specs, train, val, items, data, fp = long_case
    state = np.random.get_state()
    try:
        runs = []
        for kw in ({}, dict(augment=None), dict(augment=dict(gain_db=0.0))):
            tr = DCUE(feature_dim=32, conv_hidden=32, batch_size=8, neg_batch_size=3, lr=1e-3, device=DEV, crop="epoch",
                      crop_seed=4, **kw)
            tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
            torch.manual_seed(7)
            tr._init_nn()
            tr._bind_items(items)
            res = _sub_epoch(tr, train, 1)
            assert not tr._tracks_dirty
            runs.append((res, {k: v.detach().clone() for k, v in tr.model.state_dict().items()}, tr._tracks.clone(),
                         int(np.random.randint(0, 2 ** 31))))
            tr._plan.close()
        want = R.crop(data, fp, None, np.float16, R.RANDOM, seed=4, draw=1)[0]
        for run in runs:
            assert run[0] == runs[0][0] and run[3] == runs[0][3]
            assert np.array_equal(T._bits(run[2]), T._bits(want))
            for k in run[1]:
                assert torch.equal(run[1][k], runs[0][1][k]), k
        assert "user_embd.embeddings.weight" in runs[0][1]
    finally:
        np.random.set_state(state)


def test_constructor_refusals_and_forms(long_case):
    from dcrecommend.nn.dcue import DCUE, Augment
    with pytest.raises(ValueError, match="crop='epoch'"):
        DCUE(device=DEV, crop="load", augment=AUG)
    with pytest.raises(ValueError, match="crop='epoch'"):
        DCUE(device=DEV, augment=Augment(gain_db=3.0))  # crop defaults to 'load'
    for bad, word in ((dict(freq_masks=5), "freq_masks"), (dict(freq_masks=-1), "freq_masks"),
                      (dict(freq_width=129), "freq_width"), (dict(time_masks=5), "time_masks"),
                      (dict(time_width=132), "time_width"), (dict(time_width=1.5), "time_width"),
                      (dict(gain_db=-1.0), "gain_db"), (dict(gain_db=float("inf")), "gain_db"),
                      (dict(gain_db=float("nan")), "gain_db"), (dict(gain_db="loud"), "gain_db"),
                      (dict(fill="median"), "fill"), (dict(fill=float("nan")), "fill"), (dict(fill=None), "fill"),
                      (dict(pitch_shift=2), "unknown"), ([2, 27], "Augment")):
        with pytest.raises(ValueError, match=word):
            DCUE(device=DEV, crop="epoch", augment=bad)
    tr = DCUE(device=DEV, crop="epoch", augment=Augment(freq_masks=4, freq_width=128, time_masks=4, time_width=131,
                                                        gain_db=20, fill=-80))
    assert tr.augment == dict(freq_masks=4, freq_width=128, time_masks=4, time_width=131, gain_db=20.0, fill=-80.0)
    assert DCUE(device=DEV, crop="epoch", augment=dict(gain_db=3)).augment["fill"] == "mean"


def test_checkpoint_keeps_the_augment(long_case, tmp_path):
    from dcrecommend.nn.dcue import DCUE
    g, specs, train, val, items, data, fp = long_case
    tr = T._trainer(train, "epoch", crop_seed=11, augment=dict(fill=-80.0, **AUG))
    tr.nn_epoch = 3
    tr.save(models_dir=str(tmp_path))
    sub = tmp_path / tr._format_model_subdir()
    ck = torch.load(str(sub / "epoch_3.pth"), weights_only=True)
    assert ck["augment"] == dict(fill=-80.0, **AUG)
    tr2 = DCUE(device=DEV)
    tr2.load(str(sub), 3)
    assert tr2.augment == tr.augment and tr2.crop == "epoch"
    del ck["augment"]  # a checkpoint from before the augmentation loads without one
    torch.save(ck, str(sub / "epoch_2.pth"))
    tr3 = DCUE(device=DEV, crop="epoch", augment=AUG)
    tr3.load(str(sub), 2)
    assert tr3.augment is None


def test_train_dcue_driver_with_augment_flags(tmp_path, capsys):
    """train_dcue.py with the flags end to end on synthetic files: they reach the trainer, the settings
    print echoes them, and the run trains and checkpoints as the default does."""
    import train_dcue
    dcue = train_dcue.main(["--synthetic", "--synthetic-users", "24", "--synthetic-tracks", "80",
                            "--synthetic-pairs", "300", "--feature-dim", "32", "--conv-hidden", "32",
                            "--batch-size", "8", "--neg-batch-size", "3", "--num-epochs", "1",
                            "--eval-pct", "1.0", "--lr", "1e-3", "--save-dir", str(tmp_path),
                            "--crop", "epoch", "--crop-seed", "2", "--augment-freq-masks", "2",
                            "--augment-freq-width", "27", "--augment-time-masks", "2", "--augment-time-width", "40",
                            "--augment-gain-db", "6", "--augment-fill", "mean"])
    assert dcue.augment == dict(fill="mean", **AUG)
    assert dcue._store is not None and not dcue._tracks_dirty  # the last reader was an evaluation
    assert dcue._plan_n == 3 and dcue.nn_epoch >= 9 and 0.0 <= dcue.best_val_auc <= 1.0
    assert "Augment: freq_masks=2, freq_width=27" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        train_dcue.parse(["--synthetic", "--augment-gain-db", "6"])  # needs --crop epoch
