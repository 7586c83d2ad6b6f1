"""dcue_logmel on the GPU against the fp64 oracle of logmel_reference.py: parity in the linear, dB and
log1p domains at 4x the measured f32 distances, the bit-exact invariances include/dcue.h promises,
exact floors, flags, and the layers above it (audio.LogMel, DCUE.embed_audio and the two list calls)."""
import ctypes
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import logmel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
N_FFTS = (256, 512, 1024, 2048)
FRAMES_PER_WG = 16  # csrc/logmel.hip kLogmelFramesPerWg: frames one workgroup owns, counted from frame0


def _lm(**kw):
    from dcrecommend import audio
    return audio.LogMel(device=DEV, **kw)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def _batch(n_samples):
    """37 clips cycling through every generator (clip c: generator c % 6, its row c // 6 -- so the three
    impulse positions all occur), and each clip's generator name."""
    names = [R.LINEAR_INPUTS[c % len(R.LINEAR_INPUTS)] for c in range(37)]
    rows = {name: R.make_input(name, 7, n_samples, SR) for name in R.LINEAR_INPUTS}
    x = np.stack([rows[names[c]][c // len(R.LINEAR_INPUTS)] for c in range(37)])
    return x, names  # shared: the tests copy before they change a sample


@functools.lru_cache(maxsize=None)
def _oracle_power(n_fft, hop, n_samples):
    """fp64 mel power of _batch(n_samples), computed once per shape and shared (read-only)."""
    x, _ = _batch(n_samples)
    P = np.concatenate([R.mel_power(x[c:c + 1], SR, n_fft, hop) for c in range(len(x))])
    P.setflags(write=False)
    return P


def _sizes(n_fft):
    return (n_fft // 2 + 1, 4097, 66560)


GRID = [(n_fft, hop) for n_fft in N_FFTS for hop in (n_fft // 2, 160)]


# ------------------------------------------------------------------------------- 1. linear parity
@pytest.mark.parametrize("n_fft,hop", GRID)
def test_parity_power(n_fft, hop):
    """Mel power within 4 D_LIN of the oracle, per frame relative to the frame's largest bin, for
    n_samples in {n_fft/2+1, 4097, 66560} x clips in {1, 3, 37} and every generator. 4x: the kernel's
    butterfly and mel summation orders differ from the float32 route D_LIN was measured on; the
    rounding is of the same kind."""
    lm = _lm(n_fft=n_fft, hop=hop, compress="power")
    for n_samples in _sizes(n_fft):
        x, _ = _batch(n_samples)
        want = _oracle_power(n_fft, hop, n_samples)
        for n in (1, 3, 37):
            got = lm.transform(x[:n]).cpu().numpy()
            assert got.shape == want[:n].shape
            dist = R.frame_distance(got, want[:n])
            print("n_fft %d hop %d n_samples %d clips %d: distance %.3e (bound %.3e)"
                  % (n_fft, hop, n_samples, n, dist, 4 * R.D_LIN))
            assert dist <= 4 * R.D_LIN, (n_samples, n, dist)


# --------------------------------------------------------------------------- 2. dB / log1p parity
@pytest.mark.parametrize("n_fft,hop", GRID)
def test_parity_db_and_log1p(n_fft, hop):
    """The noise-floored clips of the same batches: |dB - oracle| <= 4 D_DB at amin = parity_amin (the
    oracle's dB output spans less than 80 dB, asserted) and |log1p - oracle| <= 4 D_L1P."""
    amin = R.parity_amin(n_fft)
    db = _lm(n_fft=n_fft, hop=hop, compress="db", amin=amin)
    l1p = _lm(n_fft=n_fft, hop=hop, compress="log1p")
    for n_samples in _sizes(n_fft):
        x, names = _batch(n_samples)
        keep = np.array([nm in R.FLOORED_INPUTS for nm in names])
        P = _oracle_power(n_fft, hop, n_samples)[keep]
        assert 20.0 < R.dynamic_range_db(P, amin) < 80.0
        for n in (1, 3, 37):
            k = keep[:n]
            e_db = np.abs(db.transform(x[:n]).cpu().numpy()[k] - R.compress(P[:k.sum()], R.DB, amin=amin)).max()
            e_l1p = np.abs(l1p.transform(x[:n]).cpu().numpy()[k] - R.compress(P[:k.sum()], R.LOG1P)).max()
            print("n_fft %d hop %d n_samples %d clips %d: dB %.3e (bound %.3e), log1p %.3e (bound %.3e)"
                  % (n_fft, hop, n_samples, n, e_db, 4 * R.D_DB, e_l1p, 4 * R.D_L1P))
            assert e_db <= 4 * R.D_DB and e_l1p <= 4 * R.D_L1P, (n_samples, n, e_db, e_l1p)


# ------------------------------------------------------------------------- 3. bit-exact properties
@pytest.mark.parametrize("n_fft,hop", [(1024, 512), (256, 160), (2048, 1024)])
def test_rows_do_not_depend_on_the_batch(n_fft, hop):
    lm = _lm(n_fft=n_fft, hop=hop)
    x, _ = _batch(66560)
    clip = x[1:2]
    alone = _bits(lm.transform(clip))
    first = np.concatenate([clip, x[5:7]])
    last = np.concatenate([x[:36], clip])
    assert np.array_equal(_bits(lm.transform(first))[0], alone[0])
    assert np.array_equal(_bits(lm.transform(last))[36], alone[0])
    assert np.array_equal(_bits(lm.transform(clip)), alone)  # two runs


@pytest.mark.parametrize("n_fft,hop", [(1024, 512), (512, 160)])
def test_frame_ranges_are_slices(n_fft, hop):
    lm = _lm(n_fft=n_fft, hop=hop)
    x, _ = _batch(66560)
    x = x[:3]
    full = _bits(lm.transform(x))
    W = FRAMES_PER_WG
    ranges = [(f0, n) for f0 in (0, 1, 65) for n in (1, 2, 66)]
    ranges += [(W - 1, 1), (W - 1, 2), (W, 1), (W + 1, 1), (0, W - 1), (0, W), (0, W + 1), (3, W), (3, W + 1),
               (full.shape[1] - 1, 1), (full.shape[1] - W - 1, W + 1)]
    for f0, n in ranges:
        got = lm.transform(x, frame0=f0, n_frames=n)
        assert got.shape == (3, n, 128)
        assert np.array_equal(_bits(got), full[:, f0:f0 + n]), (f0, n)
    assert lm.transform(x, frame0=5, n_frames=0).shape == (3, 0, 128)
    with pytest.raises(ValueError, match="frame range"):
        lm.transform(x, frame0=full.shape[1] - 1, n_frames=2)


@pytest.mark.parametrize("compress", ["db", "log1p", "power"])
def test_half_output_is_the_rounded_float_output(compress):
    lm = _lm(compress=compress)
    x, _ = _batch(66560)
    f32 = lm.transform(x[:6])
    f16 = lm.transform(x[:6], dtype=torch.float16)
    assert f16.dtype == torch.float16
    assert np.array_equal(_bits(f16), _bits(f32.half()))


# --------------------------------------------------------------------------------- 4. exact values
@pytest.mark.parametrize("n_fft", N_FFTS)
def test_silence_gives_the_floor(n_fft):
    x = R.silence(2, 4097)
    assert torch.all(_lm(n_fft=n_fft, hop=160).transform(x) == -100.0)
    assert torch.all(_lm(n_fft=n_fft, hop=160, compress="log1p").transform(x) == 0.0)
    assert torch.all(_lm(n_fft=n_fft, hop=160, compress="power").transform(x) == 0.0)
    assert torch.all(_lm(n_fft=n_fft, hop=160, amin=1e-3).transform(x) == -30.0)


def test_empty_filters_hold_the_floor():
    count = R.filter_ranges(R.filterbank(SR, 256))[1]
    empty = torch.from_numpy(count == 0)
    assert int(empty.sum()) == 20
    x, _ = _batch(4097)
    db = _lm(n_fft=256, hop=128).transform(x).cpu()
    assert torch.all(db[:, :, empty] == -100.0)
    assert torch.all(_lm(n_fft=256, hop=128, compress="power").transform(x).cpu()[:, :, empty] == 0.0)
    noisy = np.array([nm == "white_noise" for nm in _batch(4097)[1]])
    assert torch.all(db[torch.from_numpy(noisy)][:, :, ~empty] > -100.0)


# --------------------------------------------------------------------------------------- 5. flags
def test_nonfinite_samples_flag_their_clip_only():
    from dcrecommend import _native as nat
    lm = _lm()
    x = np.array(_batch(66560)[0][:3])
    clean, cflags = lm.transform_raw(x)
    assert not cflags.any()
    x[1, 1000] = np.nan
    x[1, 40000] = np.inf
    out, flags = lm.transform_raw(x)
    assert flags.tolist() == [0, nat.LOGMEL_FLAG_NONFINITE, 0]
    assert np.array_equal(_bits(out[0]), _bits(clean[0])) and np.array_equal(_bits(out[2]), _bits(clean[2]))
    with pytest.raises(ValueError, match=r"clip 1\b"):
        lm.transform(x)
    # the flags of an earlier call do not linger
    assert not lm.transform_raw(x[[0, 2]])[1].any()


# -------------------------------------------------------------------------------- 6 - 8. the layers
def _datasets(g, tmp_path):
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    from dcrecommend.datasets.dcuepredset import DCUEPredset
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
    """A tiny model with factors, built the way tests/test_gpu_topk.py builds its own."""
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    train, val, items = _datasets(g, tmp_path_factory.mktemp("mel"))
    tr = DCUE(feature_dim=int(g["d"]), conv_hidden=int(g["H"]), batch_size=8, device=DEV)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    tr._init_nn()
    tr.model.load_state_dict({k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd.")})
    tr._user_factors(items)
    tr._item_factors(items)
    tr.train_data = train
    return g, tr, train, val, items


def _clips(n=5):
    return np.array(_batch(66560)[0][:n])


def test_track_rows_feed_the_item_tower(trained):
    """track_rows is a dcue_tracks table as it stands: dcue_item_tower_eval on it gives embed_audio's
    factors bit for bit; reference_tensor is the transpose of transform."""
    from dcrecommend import _native as nat
    g, tr, train, val, items = trained
    lm = _lm()
    x = _clips()
    table = lm.track_rows(x)
    assert table.shape == (5, 131, 128) and table.dtype == torch.float16 and table.is_contiguous()
    n = table.shape[0]
    dims = tr.model._flat["dims"]
    feat = torch.empty((n, nat.storage_dims(dims).feature_dim), device=DEV)
    ws = torch.empty(nat.workspace_bytes(dims, 1, 0, n), dtype=torch.uint8, device=DEV)
    it = torch.arange(n, dtype=torch.int32, device=DEV)
    tracks = nat.Tracks(table.data_ptr(), n, 0, 0)
    model = tr.model._model_struct()
    tr.model.eval()
    nat.check(nat.lib().dcue_item_tower_eval(ctypes.byref(model), ctypes.byref(tracks), nat.ptr(it), n, nat.ptr(ws),
                                             ws.numel(), nat.ptr(feat), nat.stream_handle()), "dcue_item_tower_eval")
    got = tr.embed_audio(x, logmel=lm)
    assert got.shape == (5, tr.feature_dim) and got.is_cuda
    assert np.array_equal(_bits(got), _bits(feat[:, :tr.feature_dim]))
    assert np.array_equal(_bits(tr.embed_audio(x)), _bits(got))  # the default front end is LogMel()
    assert np.array_equal(_bits(tr.embed_audio(x[2])), _bits(got[2:3]))  # one clip, 1-D
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    # a later window of a longer clip
    long = np.concatenate([x[:2], x[2:4]], axis=1)
    f1 = lm.n_frames(long.shape[1]) - 131
    assert np.array_equal(_bits(tr.embed_audio(long, frame0=f1)),
                          _bits(tr.embed_audio(long[:, f1 * 512 - 512:], frame0=1)))
    ref = lm.reference_tensor(x)
    assert ref.shape == (5, 128, 131) and ref.is_contiguous()
    assert np.array_equal(_bits(ref), _bits(lm.transform(x).transpose(1, 2)))
    with pytest.raises(ValueError, match="clip 0"):
        tr.embed_audio(np.full(66560, np.nan, dtype=np.float32))
    with pytest.raises(ValueError, match="frame range"):
        tr.embed_audio(x[:, :66000])


def test_list_calls_are_topk_on_the_audio_factors(trained):
    from dcrecommend.nn import rank
    g, tr, train, val, items = trained
    x = _clips()
    q = tr.embed_audio(x)
    cand = tr._item_feat_by_index()
    for ds, k in ((None, 10), (val, 3), (None, 128)):
        want = rank.TopK(None, None, tr._cand_mask(ds), DEV).topk(q, cand, np.arange(5), k)
        names = tr._index_source(ds).itemindex2songid
        got = tr.similar_to_audio(x, k=k, dataset=ds)
        assert len(got) == 5
        for r in range(5):
            c = int(want[2][r])
            assert c == min(k, int(tr._cand_mask(ds).sum())) == len(got[r])
            assert [s for s, _ in got[r]] == [names[int(i)] for i in want[0][r, :c]]
            assert np.array_equal(np.array([v for _, v in got[r]], np.float32).view(np.int32),
                                  want[1][r, :c].view(np.int32))
    # the same shapes and k handling as similar_songs
    songs = list(g["val_songs"][:5])
    assert [len(l) for l in tr.similar_to_audio(x, k=10)] == [len(l) for l in tr.similar_songs(songs, k=10)]
    with pytest.raises(ValueError, match="k must be"):
        tr.similar_to_audio(x, k=129)
    n_users = tr.user_factors.shape[0]
    for k in (1, 10):
        want = rank.TopK(None, None, None, DEV, n_cand=n_users).topk(q, tr.user_factors, np.arange(5), k)
        got = tr.listeners_for_audio(x, k=k)
        for r in range(5):
            c = int(want[2][r])
            assert c == min(k, n_users) == len(got[r])
            assert [u for u, _ in got[r]] == [train.userindex2userid[int(i)] for i in want[0][r, :c]]
            assert np.array_equal(np.array([v for _, v in got[r]], np.float32).view(np.int32),
                                  want[1][r, :c].view(np.int32))
            assert all(a[1] >= b[1] for a, b in zip(got[r], got[r][1:]))


def test_audio_calls_leave_no_state_behind(trained):
    g, tr, train, val, items = trained
    users, songs = list(g["val_users"][:4]), list(g["val_songs"][:4])

    def snapshot():
        return (tr.recommend(users, k=10, dataset=val), tr.recommend(users, k=5), tr.similar_songs(songs, k=10),
                tr.evaluate_topk(ks=(5, 10)), tr.evaluate_topk(dataset=val, ks=(10,)))
    before = snapshot()
    uf, itf = tr.user_factors.clone(), tr.item_factors.clone()
    x = _clips(3)
    tr.embed_audio(x)
    tr.similar_to_audio(x, k=4)
    tr.listeners_for_audio(x, k=4)
    assert snapshot() == before
    assert torch.equal(tr.user_factors, uf) and torch.equal(tr.item_factors, itf)


def test_top_db_clamps_each_clip_at_its_own_maximum():
    x, names = _batch(66560)
    keep = np.array([nm in R.FLOORED_INPUTS for nm in names])
    # clips with different maxima: each is clamped at its own
    x = x[keep][:6] * np.array([1.0, 0.1, 1.0, 0.01, 1.0, 1.0], dtype=np.float32)[:, None]
    want = R.logmel(x, R.DB, top_db=80.0)
    got = _lm(top_db=80).transform(x).cpu().numpy()
    err = np.abs(got - want).max()
    print("top_db: %.3e (bound %.3e)" % (err, 4 * R.D_DB))
    assert err <= 4 * R.D_DB
    assert np.all(got.min(axis=(1, 2)) >= got.max(axis=(1, 2)) - 80.0)
    tight = _lm(top_db=20).transform(x).cpu().numpy()
    assert np.array_equal(tight.min(axis=(1, 2)), tight.max(axis=(1, 2)) - np.float32(20.0))


def test_transform_audio_driver(tmp_path):
    """transform_audio.py: wave files in, one [128, T] tensor per file and the metadata CSV out."""
    import wave

    import transform_audio
    from dcrecommend import audio
    x, _ = _batch(66560)
    clips = {"b_song": x[1], "a_song": x[3], "short": x[0][:4097]}
    os.makedirs(tmp_path / "wav")
    for name, c in clips.items():
        with wave.open(str(tmp_path / "wav" / (name + ".wav")), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR)
            f.writeframes(np.clip(np.round(c * 32768.0), -32768, 32767).astype("<i2").tobytes())
    meta_path = tmp_path / "metadata.csv"
    assert transform_audio.main(["--wav-dir", str(tmp_path / "wav"), "--out-dir", str(tmp_path / "mel"),
                                 "--metadata", str(meta_path), "--device", DEV]) == 0
    meta = pd.read_csv(meta_path)
    assert list(meta.columns) == ["idx", "song_id", "data_mel"]
    assert list(meta["song_id"]) == ["a_song", "b_song", "short"]
    lm = _lm()
    for song, path in zip(meta["song_id"], meta["data_mel"]):
        got = torch.load(path, weights_only=True)
        wav, rate = audio.read_wav(tmp_path / "wav" / (song + ".wav"))
        assert rate == SR and got.dtype == torch.float32
        assert got.shape == (128, 131 if song != "short" else 1 + 4097 // 512)
        assert np.array_equal(_bits(got), _bits(lm.reference_tensor(wav)[0]))
    with pytest.raises(ValueError, match="sample rate"):
        transform_audio.main(["--wav-dir", str(tmp_path / "wav"), "--out-dir", str(tmp_path / "mel2"),
                              "--metadata", str(meta_path), "--sample-rate", "16000", "--device", DEV])
