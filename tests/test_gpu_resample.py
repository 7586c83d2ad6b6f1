"""dcue_resample on the GPU against the fp64 oracle of resample_reference.py: parity at 4x the measured
f32 distance, tile edges and output ranges, the bit-exact invariances include/dcue.h promises, zero
extension, 64-bit indices, non-finite samples, and the layers above it (audio.Resampler, LogMel's
source_rate, DCUE.embed_audio's sample_rate and the transform_audio driver)."""
import functools
import os
import wave

import numpy as np
import pandas as pd
import pytest
import torch

import logmel_reference as LR
import resample_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 64  # csrc/resample.hip kResampleTile: outputs one workgroup owns, counted from out0
GRID = [(ri, ro, q) for ri, ro in R.PAIRS for q in ("best", "fast")]


def _ids(v):
    return "%d-%d-%s" % v


@functools.lru_cache(maxsize=None)
def _rs(ri, ro, quality="best"):
    from dcrecommend import audio
    return audio.Resampler(ri, ro, quality, device=DEV)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def _batch(n_in, rate):
    return R.batch(n_in, rate)  # shared: the tests copy before they change a sample


@functools.lru_cache(maxsize=None)
def _oracle(ri, ro, quality, n_in):
    y = R.resample(_batch(n_in, ri)[0], ri, ro, quality)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_parity(case):
    """Every clip within 4 D_RS of the oracle (max |y - oracle| over the clip's largest |oracle|) for
    n_in in {1, Kh - 1, K + 1, 4097} x clips in {1, 3, 37} and every generator; silence gives exact zeros.
    4x: the kernel's summation order (one ascending chain) differs from the float32 route D_RS was measured
    on; the rounding is of the same kind."""
    ri, ro, quality = case
    rs = _rs(ri, ro, quality)
    for n_in in R.parity_sizes(ri, ro, quality):
        x, names = _batch(n_in, ri)
        want = _oracle(ri, ro, quality, n_in)
        for n in (1, 3, 37):
            got = rs.resample(x[:n]).cpu().numpy()
            assert got.shape == want[:n].shape == (n, rs.n_out(n_in))
            dist = R.clip_distance(got, want[:n])
            print("%d -> %d %s n_in %d clips %d: distance %.3e (bound %.3e)"
                  % (ri, ro, quality, n_in, n, dist.max(), 4 * R.D_RS))
            assert dist.max() <= 4 * R.D_RS, (n_in, n, int(dist.argmax()), dist.max())
            for c in range(n):
                if names[c] == "silence":
                    assert not got[c].any()


# --------------------------------------------------------------------------------- 2. tile edges
@pytest.mark.parametrize("ri,ro", [(44100, 22050), (48000, 22050)])
def test_tile_edges_and_output_ranges(ri, ro):
    L, M, K, Kh, _ = R.shape(ri, ro)
    rs = _rs(ri, ro)
    for target in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        n_in = ((target - 1) * M) // L + 1
        assert rs.n_out(n_in) == target
        x = LR.white_noise(3, n_in, seed=target)
        dist = R.clip_distance(rs.resample(x).cpu().numpy(), R.resample(x, ri, ro)).max()
        print("%d -> %d n_out %d: distance %.3e" % (ri, ro, target, dist))
        assert dist <= 4 * R.D_RS
    x = _batch(4097, ri)[0][:3]
    full = _bits(rs.resample(x))
    total = full.shape[1]
    T = TILE
    ranges = [(0, T - 1), (0, T), (0, T + 1), (1, T), (T - 1, 1), (T - 1, 2), (T, 1), (T + 1, 1), (3, T), (3, T + 1),
              (5, 2 * T + 7), (T, T), (total - 1, 1), (total - T - 1, T + 1), (0, 1), (total, 0)]
    for out0, n in ranges:
        got = rs.resample(x, out0=out0, n_out=n)
        assert got.shape == (3, n)
        assert np.array_equal(_bits(got), full[:, out0:out0 + n]), (out0, n)
    with pytest.raises(ValueError, match="output range"):
        rs.resample(x, out0=total - 1, n_out=2)


# ------------------------------------------------------------------------- 3. bit-exact properties
@pytest.mark.parametrize("case", [(44100, 22050, "best"), (48000, 22050, "best"), (16000, 22050, "fast")], ids=_ids)
def test_outputs_do_not_depend_on_the_batch(case):
    ri, ro, quality = case
    rs = _rs(ri, ro, quality)
    x, _ = _batch(4097, ri)
    clip = x[1:2]
    alone = _bits(rs.resample(clip))
    first = np.concatenate([clip, x[5:7]])
    last = np.concatenate([x[:36], clip])
    assert np.array_equal(_bits(rs.resample(first))[0], alone[0])
    assert np.array_equal(_bits(rs.resample(last))[36], alone[0])
    assert np.array_equal(_bits(rs.resample(clip)), alone)  # two runs
    assert np.array_equal(_bits(rs.resample(np.concatenate([x[:32], clip, x[:5]])))[32], alone[0])  # second clip block


# -------------------------------------------------------------------------------- 4. zero extension
@pytest.mark.parametrize("case", [(44100, 22050, "best"), (48000, 22050, "best"), (22050, 44100, "fast")], ids=_ids)
def test_zero_extension(case):
    ri, ro, quality = case
    L, M, K, Kh, _ = R.shape(ri, ro, quality)
    rs = _rs(ri, ro, quality)
    tab = rs.host_table()[32:].view(np.float32).reshape(L, K).astype(np.float64)
    n_in = 1000
    x = np.zeros((2, n_in), dtype=np.float32)
    x[0, 0] = x[1, n_in - 1] = 1.0
    got = rs.resample(x).cpu().numpy()
    m = np.arange(got.shape[1], dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    for c, pos in ((0, 0), (1, n_in - 1)):  # y[m] = tab[p][k] with q - Kh + 1 + k = pos
        k = pos - q + Kh - 1
        want = np.where((k >= 0) & (k < K), tab[p, np.clip(k, 0, K - 1)], 0.0)
        assert np.abs(want).max() > 0.1
        assert np.abs(got[c] - want).max() <= 4 * R.D_RS * np.abs(want).max()
    # inside a longer zero-padded buffer: the same bits on the shared outputs (front pad 3 M samples = 3 L outputs)
    clip = _batch(4097, ri)[0][1:2][:, :777]
    alone = _bits(rs.resample(clip))
    padded = np.concatenate([np.zeros((1, 3 * M), np.float32), clip, np.zeros((1, 100), np.float32)], axis=1)
    inside = _bits(rs.resample(padded))
    assert np.array_equal(inside[:, 3 * L:3 * L + alone.shape[1]], alone)


# ---------------------------------------------------------------------------------- 5. large indices
def test_indices_beyond_32_bits():
    """One 48000 -> 22050 clip of 29,500,000 samples; outputs [13,500,000, +4096): m M > 2^32."""
    ri, ro = 48000, 22050
    L, M, K, Kh, _ = R.shape(ri, ro)
    out0, n = 13_500_000, 4096
    assert out0 * M > 2 ** 32
    x = (0.1 * np.random.RandomState(5).standard_normal(29_500_000)).astype(np.float32)[None, :]
    got = _rs(ri, ro).resample(torch.from_numpy(x), out0=out0, n_out=n).cpu().numpy()
    # the oracle on that range only: a slice of the clip that starts a whole number of blocks (M samples =
    # L outputs) before the range's window keeps every output's phase
    j = (out0 * M // L - Kh) // M
    lo, hi = j * M, (out0 + n) * M // L + Kh + 2
    want = R.resample(x[:, lo:hi], ri, ro, "best", out0 - j * L, n)
    dist = R.clip_distance(got, want).max()
    print("outputs %d..%d of a %d-sample clip: distance %.3e" % (out0, out0 + n, x.shape[1], dist))
    assert dist <= 4 * R.D_RS


# ------------------------------------------------------------------------------------ 6. non-finite
@pytest.mark.parametrize("ri,ro,bad", [(44100, 22050, np.nan), (48000, 22050, np.inf), (22050, 44100, -np.inf)])
def test_nonfinite_samples_reach_their_outputs_only(ri, ro, bad):
    from dcrecommend import audio
    L, M, K, Kh, _ = R.shape(ri, ro)
    rs = _rs(ri, ro)
    x = np.array(_batch(4097, ri)[0][:3])
    clean = rs.resample(x)
    assert torch.isfinite(clean).all()
    pos = 2345
    x[1, pos] = bad
    out = rs.resample(x)
    m = np.arange(out.shape[1], dtype=np.int64)
    q = (m * M) // L
    covered = (q - Kh + 1 <= pos) & (pos <= q + Kh)
    assert abs(covered.sum() - K * L / M) <= 1  # K windows hold the sample, L / M outputs per window start
    assert np.array_equal(~torch.isfinite(out[1]).cpu().numpy(), covered)
    assert np.array_equal(_bits(out[1])[~covered], _bits(clean[1])[~covered])
    assert np.array_equal(_bits(out[0]), _bits(clean[0])) and np.array_equal(_bits(out[2]), _bits(clean[2]))
    lm = audio.LogMel(device=DEV, sample_rate=ro)
    with pytest.raises(ValueError, match=r"clip 1\b"):
        lm.transform(x, source_rate=ri)


# -------------------------------------------------------------------------------------- 7. layers
def test_equal_rates_return_the_input():
    from dcrecommend import _native as nat
    from dcrecommend import audio
    x = torch.from_numpy(LR.white_noise(2, 500)).to(DEV)
    launches = nat.lib().dcue_launch_count()
    assert audio.Resampler(22050, 22050, device=DEV).resample(x) is x
    assert nat.lib().dcue_launch_count() == launches


def test_logmel_source_rate_is_resample_then_transform():
    from dcrecommend import audio
    lm = audio.LogMel(device=DEV)
    x44 = _batch(133120, 44100)[0][:5]
    for quality in ("best", "fast"):
        y = _rs(44100, 22050, quality).resample(x44)
        assert y.shape == (5, 66560)
        assert np.array_equal(_bits(lm.transform(x44, source_rate=44100, resample=quality)), _bits(lm.transform(y)))
    y = _rs(44100, 22050).resample(x44)
    assert np.array_equal(_bits(lm.transform(x44, frame0=3, n_frames=7, source_rate=44100)),
                          _bits(lm.transform(y, frame0=3, n_frames=7)))
    assert np.array_equal(_bits(lm.track_rows(x44, source_rate=44100)), _bits(lm.track_rows(y)))
    assert np.array_equal(_bits(lm.reference_tensor(x44, source_rate=44100)), _bits(lm.reference_tensor(y)))
    x22 = _batch(66560, 22050)[0][:2]
    assert np.array_equal(_bits(lm.transform(x22, source_rate=22050)), _bits(lm.transform(x22)))  # nothing to do


def test_tone_pair_survives_the_rate_change():
    """1 kHz + 3 kHz generated at 22,050 Hz and at 44,100 Hz: the mel power of the resampled clip is within
    2 x D_TONE_PAIR (what the two fp64 oracles give) + 4 D_LIN of the direct clip's, over the frames that do
    not touch the clip's ends."""
    from dcrecommend import audio
    lm = audio.LogMel(device=DEV, compress="power")
    direct = lm.transform(R.tone_pair(66560, 22050)).cpu().numpy()
    via = lm.transform(R.tone_pair(133120, 44100), source_rate=44100).cpu().numpy()
    assert direct.shape == via.shape == (1, 131, 128)
    d = LR.frame_distance(via[:, 2:-2], direct[:, 2:-2].astype(np.float64))
    bound = 2 * R.D_TONE_PAIR + 4 * LR.D_LIN
    print("tone pair: frame distance %.3e (bound %.3e)" % (d, bound))
    assert d <= bound


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
    return DCUEPredset(trip.copy(), meta, split="train"), DCUEItemset(trip.copy(), meta)


@pytest.fixture(scope="module")
def trained(golden, tmp_path_factory):
    """A tiny model with factors, built the way tests/test_gpu_logmel.py builds its own."""
    from dcrecommend.nn.dcue import DCUE
    g = golden("eval.npz")
    train, items = _datasets(g, tmp_path_factory.mktemp("mel"))
    tr = DCUE(feature_dim=int(g["d"]), conv_hidden=int(g["H"]), batch_size=8, device=DEV)
    tr.n_users, tr.n_items, tr.epoch_size = len(train.user_index), len(train.item_index), 64
    tr._init_nn()
    tr.model.load_state_dict({k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd.")})
    tr._user_factors(items)
    tr._item_factors(items)
    tr.train_data = train
    return tr


def test_embed_audio_takes_a_sample_rate(trained):
    tr = trained
    x44 = _batch(133120, 44100)[0][:4]
    y = _rs(44100, 22050).resample(x44)
    want = tr.embed_audio(y)
    assert np.array_equal(_bits(tr.embed_audio(x44, sample_rate=44100)), _bits(want))
    assert np.array_equal(_bits(tr.embed_audio(x44, sample_rate=44100, resample="fast")),
                          _bits(tr.embed_audio(_rs(44100, 22050, "fast").resample(x44))))
    x22 = _batch(66560, 22050)[0][:4]
    base = _bits(tr.embed_audio(x22))
    assert np.array_equal(_bits(tr.embed_audio(x22, sample_rate=None)), base)
    assert np.array_equal(_bits(tr.embed_audio(x22, sample_rate=22050, resample="fast")), base)
    # a longer clip, every frame: crops over the resampled clip
    x44l = _batch(133120 * 2, 44100)[0][:2]
    assert np.array_equal(_bits(tr.embed_audio(x44l, crops=3, sample_rate=44100)),
                          _bits(tr.embed_audio(_rs(44100, 22050).resample(x44l), crops=3)))
    assert tr.similar_to_audio(x44, k=5, sample_rate=44100) == tr.similar_to_audio(y, k=5)
    assert tr.listeners_for_audio(x44, k=5, sample_rate=44100) == tr.listeners_for_audio(y, k=5)
    assert tr.similar_to_audio(x44, k=5, sample_rate=44100) != tr.similar_to_audio(x44[:, :66560], k=5)


def _write_wav(path, data, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.clip(np.round(data * 32768.0), -32768, 32767).astype("<i2").tobytes())


def test_transform_audio_resamples_a_mixed_folder(tmp_path, trained):
    """22,050 Hz, 44,100 Hz stereo and 48,000 Hz files in one folder; then file -> similar_to_audio."""
    import transform_audio
    from dcrecommend import audio
    os.makedirs(tmp_path / "wav")
    x22 = _batch(66560, 22050)[0]
    x44 = _batch(133120, 44100)[0]
    _write_wav(tmp_path / "wav" / "a22.wav", x22[1], 22050)
    _write_wav(tmp_path / "wav" / "b44.wav", np.stack([x44[1], x44[3]], axis=1), 44100)
    _write_wav(tmp_path / "wav" / "c44.wav", np.stack([x44[3], x44[7]], axis=1), 44100)
    _write_wav(tmp_path / "wav" / "d48.wav", LR.tones(1, 30001, 48000)[0], 48000)
    meta_path = tmp_path / "metadata.csv"
    base = ["--wav-dir", str(tmp_path / "wav"), "--out-dir", str(tmp_path / "mel"), "--metadata", str(meta_path),
            "--device", DEV]
    with pytest.raises(ValueError, match="sample rate"):
        transform_audio.main(base)
    with pytest.raises(ValueError, match="sample rate"):
        transform_audio.main(base + ["--resample", "off"])
    lm = audio.LogMel(device=DEV)
    for quality in ("best", "fast"):
        assert transform_audio.main(base + ["--resample", quality]) == 0
        meta = pd.read_csv(meta_path)
        assert list(meta["song_id"]) == ["a22", "b44", "c44", "d48"]
        for song, path in zip(meta["song_id"], meta["data_mel"]):
            got = torch.load(path, weights_only=True)
            wav, rate = audio.read_wav(tmp_path / "wav" / (song + ".wav"))
            assert rate == {"a": 22050, "b": 44100, "c": 44100, "d": 48000}[song[0]]
            want = lm.reference_tensor(wav, source_rate=rate, resample=quality)[0]
            n22 = len(wav) if rate == 22050 else _rs(rate, 22050).n_out(len(wav))
            assert got.shape == (128, 1 + n22 // 512) and got.dtype == torch.float32
            assert np.array_equal(_bits(got), _bits(want)), song
    # from a 44.1 kHz stereo file to a list of similar songs with nothing but this package
    wav, rate = audio.read_wav(tmp_path / "wav" / "b44.wav")
    lists = trained.similar_to_audio(wav, k=3, sample_rate=rate)
    assert len(lists) == 1 and len(lists[0]) == 3
