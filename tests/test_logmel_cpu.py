"""The audio front end without a GPU: the fp64 oracle against an independent float32 route (where the
GPU tests' tolerances come from), the host-computed table against the oracle, frame counts, every
refusal of include/dcue.h, the ABI mirror, the kernels' resources, and the wave-file reader."""
import ctypes
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import logmel_reference as R
from conftest import ROOT
from kernel_resources import kernel_resources

N_FFTS = (256, 512, 1024, 2048)
SR = 22050


def _hops(n_fft):
    return (n_fft // 2, 160)


def _sizes(n_fft):
    return (n_fft // 2 + 1, 4097, 66560)


# --------------------------------------------------------------------------- oracle vs torch (1, 2)
def test_oracle_against_torch():
    """The oracle against torch's float32 CPU route on every parity input of the GPU grid. Prints the
    measured f32 distances; logmel_reference.D_LIN / D_DB / D_L1P record them (the GPU tests allow 4x).
    The float32 route's FFT differs between torch builds, so the recorded figures are held to a factor
    of two of what this machine measures, not to equality."""
    d_lin = d_db = d_l1p = 0.0
    worst_range = 0.0
    for n_fft in N_FFTS:
        for hop in _hops(n_fft):
            for n_samples in _sizes(n_fft):
                for name in R.LINEAR_INPUTS:
                    x = R.make_input(name, 37 if n_samples < 66560 else 3, n_samples, SR)
                    P64 = R.mel_power(x, SR, n_fft, hop)
                    P32 = R.torch_route(x, SR, n_fft, hop)
                    assert P32.shape == P64.shape == (len(x), R.n_frames(n_samples, n_fft, hop), 128)
                    d_lin = max(d_lin, R.frame_distance(P32, P64))
                    if name not in R.FLOORED_INPUTS:
                        continue
                    # dynamic-range condition: the oracle's dB output spans less than 80 dB (logmel_reference.
                    # parity_amin), and the clip reaches well above the floor
                    amin = R.parity_amin(n_fft)
                    rng = R.dynamic_range_db(P64, amin)
                    worst_range = max(worst_range, rng)
                    assert 20.0 < rng < 80.0, (name, n_fft, hop, n_samples, rng)
                    P32f = P32.astype(np.float32)
                    db32 = 10.0 * np.log10(np.maximum(P32f, np.float32(amin)), dtype=np.float32)
                    d_db = max(d_db, float(np.abs(db32 - R.compress(P64, R.DB, amin=amin)).max()))
                    l32 = np.log1p(np.float32(10.0) * np.sqrt(P32f, dtype=np.float32), dtype=np.float32)
                    d_l1p = max(d_l1p, float(np.abs(l32 - R.compress(P64, R.LOG1P)).max()))
    print("measured f32 distances: D_LIN %.3e  D_DB %.3e  D_L1P %.3e  (largest dynamic range %.1f dB)"
          % (d_lin, d_db, d_l1p, worst_range))
    for got, rec in ((d_lin, R.D_LIN), (d_db, R.D_DB), (d_l1p, R.D_L1P)):
        assert rec / 2 <= got <= rec * 2, (got, rec)


def test_pure_tone_is_linear_only():
    """A pure tone has far more than 80 dB of dynamic range: it belongs in the linear test alone."""
    assert "pure_tones" in R.LINEAR_INPUTS and "pure_tones" not in R.FLOORED_INPUTS
    P = R.mel_power(R.make_input("pure_tones", 1, 66560, SR), SR, 1024, 512)
    assert R.dynamic_range_db(P) > 100.0


def test_default_clip_is_a_track():
    assert R.n_frames(66560, 1024, 512) == 131


# ------------------------------------------------------------------------------ the library
def _lm(**kw):
    from dcrecommend import audio
    return audio.LogMel(**kw)


def _parse(table, n_fft):
    M = n_fft // 2
    H = M // 2 + 1
    hdr = table[:32].view(np.int32)
    o = 32
    win = table[o:o + 4 * n_fft].view(np.float32); o += 4 * n_fft
    twm = table[o:o + 8 * M].view(np.float32).reshape(M, 2); o += 8 * M
    twn = table[o:o + 8 * H].view(np.float32).reshape(H, 2); o += 8 * H
    rng = table[o:o + 12 * 128].view(np.int32).reshape(3, 128); o += 12 * 128
    wts = table[o:o + 4 * (n_fft + 2)].view(np.float32); o += 4 * (n_fft + 2)
    assert o == len(table)
    return hdr, win, twm, twn, rng, wts


def _within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("n_fft,sr,fmin,fmax", [(256, SR, 0.0, None), (512, SR, 0.0, None), (1024, SR, 0.0, None),
                                                (2048, SR, 0.0, None), (1024, 16000, 30.0, 7600.0)])
def test_host_table_matches_oracle(n_fft, sr, fmin, fmax):
    lm = _lm(sample_rate=sr, n_fft=n_fft, hop=n_fft // 2, fmin=fmin, fmax=fmax)
    hdr, win, twm, twn, rng, wts = _parse(lm.host_table(), n_fft)
    first, count, packed = R.filter_ranges(R.filterbank(sr, n_fft, fmin, fmax))
    assert hdr[1] == n_fft and hdr[2] == len(packed) <= n_fft + 2
    assert np.array_equal(rng[0], first) and np.array_equal(rng[1], count)  # the ranges: exactly
    assert np.array_equal(rng[2], np.concatenate([[0], np.cumsum(count)[:-1]]))
    _within_one_ulp(wts[:len(packed)], packed)
    assert not wts[len(packed):].any()
    _within_one_ulp(win, R.hann(n_fft))
    M = n_fft // 2
    t = np.arange(M) / M
    _within_one_ulp(twm, np.stack([np.cos(2 * np.pi * t), -np.sin(2 * np.pi * t)], 1))
    k = np.arange(M // 2 + 1) / n_fft
    _within_one_ulp(twn, np.stack([np.cos(2 * np.pi * k), -np.sin(2 * np.pi * k)], 1))
    if n_fft == 256 and sr == SR:
        assert int((count == 0).sum()) == 20  # narrower than the FFT's resolution: legal, they hold the floor
    if n_fft >= 1024 and sr == SR:
        assert count.min() > 0 and count.max() == {1024: 26, 2048: 53}[n_fft]


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft", N_FFTS)
def test_frame_counts(n_fft, center):
    for hop in _hops(n_fft) + (1, n_fft):
        lm = _lm(n_fft=n_fft, hop=hop, center=center)
        for n in (n_fft // 2 + 1, n_fft, 4096, 4097, 66559, 66560, 66561):
            if not center and n < n_fft:
                with pytest.raises(ValueError, match="center = 0"):
                    lm.n_frames(n)
            else:
                assert lm.n_frames(n) == R.n_frames(n, n_fft, hop, center), (hop, n)


def _cfg(**kw):
    from dcrecommend import _native as nat
    v = dict(sample_rate=SR, n_fft=1024, hop=512, center=1, compress=nat.LOGMEL_DB, out_dtype=1, fmin=0.0,
             fmax=SR / 2.0, amin=1e-10, log_scale=10.0)
    v.update(kw)
    return nat.LogmelConfig(*[v[f] for f, _ in nat.LogmelConfig._fields_])


BAD_CONFIGS = [(dict(n_fft=128), "n_fft"), (dict(n_fft=1000), "n_fft"), (dict(n_fft=4096), "n_fft"),
               (dict(hop=0), "hop"), (dict(hop=1025), "hop"), (dict(fmin=-1.0), "fmin"),
               (dict(fmax=SR / 2.0 + 1.0), "fmin"), (dict(fmin=4000.0, fmax=4000.0), "fmin"),
               (dict(fmin=5000.0, fmax=4000.0), "fmin"), (dict(amin=0.0), "amin"), (dict(amin=-1.0), "amin"),
               (dict(compress=3), "compress"), (dict(out_dtype=2), "out_dtype"), (dict(center=2), "center"),
               (dict(sample_rate=0), "sample_rate")]


@pytest.mark.parametrize("kw,word", BAD_CONFIGS)
def test_invalid_configurations_are_refused(kw, word):
    """DCUE_ERR_INVALID with a dcue_last_error text from every entry point, before any device call."""
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg(**kw)
    n, b = ctypes.c_int64(), ctypes.c_size_t()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    calls = [lambda: lib.dcue_logmel_frames(ctypes.byref(cfg), 66560, ctypes.byref(n)),
             lambda: lib.dcue_logmel_table_bytes(ctypes.byref(cfg), ctypes.byref(b)),
             lambda: lib.dcue_logmel_table_fill_host(ctypes.byref(cfg), ctypes.c_void_p(buf.ctypes.data), buf.nbytes),
             lambda: lib.dcue_logmel_table_init(ctypes.byref(cfg), ctypes.c_void_p(buf.ctypes.data), buf.nbytes, None),
             lambda: lib.dcue_logmel(ctypes.byref(cfg), ctypes.c_void_p(buf.ctypes.data),
                                     ctypes.c_void_p(buf.ctypes.data), 1, 66560, 0, 131,
                                     ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data), None)]
    for call in calls:
        assert call() == 1
        assert word in lib.dcue_last_error().decode()


def test_amin_matters_only_for_db():
    from dcrecommend import _native as nat
    n = ctypes.c_int64()
    assert nat.lib().dcue_logmel_frames(ctypes.byref(_cfg(amin=0.0, compress=nat.LOGMEL_POWER)), 66560, ctypes.byref(n)) == 0
    assert n.value == 131


@pytest.mark.parametrize("kw,n_samples,frame0,n_frames,word", [
    (dict(), 512, 0, 1, "center = 1"),            # n_samples <= n_fft / 2: the reflection is undefined
    (dict(), 1, 0, 1, "center = 1"),
    (dict(center=0), 1023, 0, 1, "center = 0"),   # not one whole frame
    (dict(), 66560, 0, 132, "frame range"),       # one frame past the clip's 131
    (dict(), 66560, 131, 1, "frame range"),
    (dict(), 66560, 1, 131, "frame range"),
    (dict(center=0), 66560, 0, 130, "frame range"),  # 129 frames without the padding
    (dict(), 66560, -1, 2, "negative"),
    (dict(), 66560, 0, -1, "negative"),
])
def test_invalid_shapes_are_refused(kw, n_samples, frame0, n_frames, word):
    """The shape refusals of dcue_logmel, reached with host memory and no GPU: the call returns before
    it reads a pointer or launches."""
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg(**kw)
    buf = np.zeros(64, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    launches = lib.dcue_launch_count()
    assert lib.dcue_logmel(ctypes.byref(cfg), p, p, 1, n_samples, frame0, n_frames, p, p, None) == 1
    assert word in lib.dcue_last_error().decode()
    assert lib.dcue_launch_count() == launches


def test_null_pointers_are_refused():
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg()
    assert lib.dcue_logmel(ctypes.byref(cfg), None, None, 1, 66560, 0, 131, None, None, None) == 1
    assert lib.dcue_logmel(None, None, None, 1, 66560, 0, 131, None, None, None) == 1
    assert lib.dcue_logmel_table_fill_host(ctypes.byref(cfg), None, 1 << 20) == 1
    small = np.zeros(64, dtype=np.uint8)
    assert lib.dcue_logmel_table_fill_host(ctypes.byref(cfg), ctypes.c_void_p(small.ctypes.data), 64) == 1


def test_python_front_end_validates_on_the_host():
    with pytest.raises(ValueError, match="n_fft"):
        _lm(n_fft=300)
    with pytest.raises(ValueError, match="compress"):
        _lm(compress="mel")
    with pytest.raises(ValueError, match="top_db"):
        _lm(compress="log1p", top_db=80)


# ------------------------------------------------------------------------------------ ABI (6)
def test_abi_and_struct(tmp_path):
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == nat.ABI_VERSION
    assert nat.lib().dcue_abi_version() == 17
    names = ["dcue_logmel_frames", "dcue_logmel_table_bytes", "dcue_logmel_table_fill_host", "dcue_logmel_table_init",
             "dcue_logmel"]
    for n in names:
        assert re.search(r"^int %s\(" % n, hdr, flags=re.M), n
        assert n in nat._SIGS and hasattr(nat.lib(), n)
    for macro, val in (("DCUE_LOGMEL_POWER", nat.LOGMEL_POWER), ("DCUE_LOGMEL_DB", nat.LOGMEL_DB),
                       ("DCUE_LOGMEL_LOG1P", nat.LOGMEL_LOG1P), ("DCUE_LOGMEL_FLAG_NONFINITE", nat.LOGMEL_FLAG_NONFINITE)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, hdr).group(1)) == val
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcue.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(dcue_logmel_config));']
    for f, _ in nat.LogmelConfig._fields_:
        src.append('printf("%s %%zu\\n", offsetof(dcue_logmel_config, %s));' % (f, f))
    src.append("return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.LogmelConfig) == 40
    for f, _ in nat.LogmelConfig._fields_:
        assert int(got[f]) == getattr(nat.LogmelConfig, f).offset, f


# ------------------------------------------------------------------------ kernel resources (7)
def test_logmel_kernels_use_no_scratch(tmp_path):
    res = {k: v for k, v in kernel_resources("logmel.hip", tmp_path).items() if "k_logmel" in k}
    assert len(res) == 4, sorted(res)  # one instance per n_fft
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 256, (name, r)


# ---------------------------------------------------------------------------------- read_wav (8)
def _write_wav(path, data, rate, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data.tobytes())


def test_read_wav_round_trip(tmp_path):
    from dcrecommend import audio
    rs = np.random.RandomState(0)
    mono = rs.randint(-32768, 32768, size=1000).astype("<i2")
    mono[:2] = (-32768, 32767)
    _write_wav(tmp_path / "m.wav", mono, SR)
    x, rate = audio.read_wav(tmp_path / "m.wav")
    assert rate == SR and x.dtype == np.float32 and x.shape == (1000,)
    assert np.array_equal(x, mono.astype(np.float32) / 32768.0)  # exact: 16 bits fit a float32
    stereo = rs.randint(-32768, 32768, size=(777, 2)).astype("<i2")
    _write_wav(tmp_path / "s.wav", stereo, 44100)
    x, rate = audio.read_wav(tmp_path / "s.wav")
    assert rate == 44100 and x.shape == (777,)
    assert np.array_equal(x, ((stereo[:, 0].astype(np.float32) + stereo[:, 1].astype(np.float32)) / 2) / 32768.0)
    assert audio.read_wav(tmp_path / "m.wav", sample_rate=SR)[1] == SR
    with pytest.raises(ValueError, match="sample rate"):
        audio.read_wav(tmp_path / "s.wav", sample_rate=SR)


@pytest.mark.parametrize("width", [1, 3])
def test_read_wav_refuses_other_widths(tmp_path, width):
    from dcrecommend import audio
    _write_wav(tmp_path / "w.wav", np.zeros(100 * width, dtype=np.uint8), SR, width)
    with pytest.raises(ValueError, match="%d-bit" % (8 * width)):
        audio.read_wav(tmp_path / "w.wav")
