"""Sample-rate conversion without a GPU: the fp64 oracle against scipy's polyphase resampler, the
filter's quality on the oracle, the float32 distance the GPU tolerance comes from, the host-computed
table against the oracle, output lengths, every refusal of include/dcue.h, the ABI mirror and the
kernel's resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import logmel_reference as LR
import resample_reference as R
from conftest import ROOT
from kernel_resources import kernel_resources

QUALITIES = ("best", "fast")
GRID = [(ri, ro, q) for ri, ro in R.PAIRS for q in QUALITIES]


def _ids(v):
    return "%d-%d-%s" % v


# ----------------------------------------------------------------------------- (a) oracle = scipy
@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_oracle_is_scipy_resample_poly(case):
    """resample_poly(x, L, M, window=hu) / L with hu the same taps on the upsampled grid: an independent
    implementation of the same filter (upfirdn) agrees to 1e-11."""
    from scipy.signal import resample_poly
    ri, ro, quality = case
    L, M, K, Kh, _ = R.shape(ri, ro, quality)
    hu = R.upsampled_fir(ri, ro, quality)
    worst = 0.0
    for n_in in (1, 2, 3, Kh - 1, K + 1, 3000):
        x = np.random.RandomState(n_in).standard_normal((2, n_in))
        want = resample_poly(x, L, M, axis=1, window=hu) / L
        got = R.resample(x, ri, ro, quality)
        assert got.shape == want.shape == (2, R.n_out(n_in, ri, ro)), (n_in, got.shape, want.shape)
        worst = max(worst, float(np.abs(got - want).max()))
    print("%d -> %d %s: oracle - scipy %.3e" % (ri, ro, quality, worst))
    assert worst <= 1e-11


def test_oracle_output_ranges_are_slices():
    x = LR.white_noise(2, 3000)
    full = R.resample(x, 48000, 22050, "fast")
    for out0, count in ((0, 1), (5, 700), (full.shape[1] - 3, 3), (17, 0)):
        assert np.array_equal(R.resample(x, 48000, 22050, "fast", out0, count), full[:, out0:out0 + count])


# ------------------------------------------------------------------------------ (b) filter quality
def _tone(freq, n, rate):
    return np.sin(2 * np.pi * freq * np.arange(n, dtype=np.float64) / rate)[None, :]


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_filter_quality(case):
    """A tone at 1.15 x the lower Nyquist frequency is rejected (<= -140 dB best, <= -85 dB fast: 6 - 12 dB
    over what the oracle measures), a 1 kHz tone passes with error <= 1e-7 / 5e-5 in the clip's middle half
    (4 - 7x over the measured 1.4e-8 / 1.2e-5), and every phase row sums to 1 within 1e-7 / 1e-4."""
    ri, ro, quality = case
    best = quality == "best"
    n_in = 12000
    if ro < ri:  # down: the tone lies above the new Nyquist frequency and must vanish
        y = R.resample(_tone(1.15 * ro / 2.0, n_in, ri), ri, ro, quality)[0]
        stop_db = 20.0 * np.log10(np.abs(y[len(y) // 4:3 * len(y) // 4]).max())
    else:  # up: no input tone lies there; the image of a tone at 0.85 x the old Nyquist does (at 1.15 x)
        y = R.resample(_tone(0.85 * ri / 2.0, n_in, ri), ri, ro, quality)[0]
        mid = y[len(y) // 4:3 * len(y) // 4]
        w = np.kaiser(len(mid), 30.0)  # side lobes below -200 dB: the tone itself does not leak in
        probe = np.exp(-2j * np.pi * (1.15 * ri / 2.0) * np.arange(len(mid)) / ro)
        stop_db = 20.0 * np.log10(max(2.0 * abs(np.sum(mid * w * probe)) / w.sum(), 1e-300))
    y = R.resample(_tone(1000.0, n_in, ri), ri, ro, quality)[0]
    err = np.abs(y - _tone(1000.0, len(y), ro)[0])[len(y) // 4:3 * len(y) // 4].max()
    dc = np.abs(R.table(ri, ro, quality).sum(axis=1) - 1.0).max()
    print("%d -> %d %s: stopband %.1f dB, passband error %.2e, DC gain error %.2e" % (ri, ro, quality, stop_db, err, dc))
    assert stop_db <= (-140.0 if best else -85.0)
    assert err <= (1e-7 if best else 5e-5)
    assert dc <= (1e-7 if best else 1e-4)


# ----------------------------------------------------------------------------------- (c) D_RS
def test_f32_distance():
    """The float32 CPU route (conv1d over the phase filters) against the oracle on every clip of the GPU
    parity grid; prints the largest per-clip distance and holds resample_reference.D_RS within a factor of
    two of it (the GPU tests allow 4x D_RS)."""
    worst = 0.0
    for ri, ro, quality in GRID:
        for n_in in R.parity_sizes(ri, ro, quality):
            x, _ = R.batch(n_in, ri)
            d = R.clip_distance(R.torch_route(x, ri, ro, quality).numpy(), R.resample(x, ri, ro, quality)).max()
            worst = max(worst, float(d))
    print("measured f32 distance: D_RS %.3e" % worst)
    assert R.D_RS / 2 <= worst <= R.D_RS * 2, (worst, R.D_RS)


def test_tone_pair_oracle_figure():
    """D_TONE_PAIR: the two fp64 oracles on the layer test's tone pair (tests/test_gpu_resample.py)."""
    n22 = 66560
    direct = LR.mel_power(R.tone_pair(n22, 22050))
    via = LR.mel_power(R.resample(R.tone_pair(2 * n22, 44100), 44100, 22050, "best"))
    assert direct.shape == via.shape
    d = LR.frame_distance(via[:, 2:-2], direct[:, 2:-2])
    print("tone pair, fp64: frame distance %.3e" % d)
    assert R.D_TONE_PAIR / 2 <= d <= R.D_TONE_PAIR * 2, (d, R.D_TONE_PAIR)


# ------------------------------------------------------------------------------ the library
def _rs(ri, ro, quality="best"):
    from dcrecommend import audio
    return audio.Resampler(ri, ro, quality)


@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_host_table_matches_oracle(case):
    ri, ro, quality = case
    L, M, K, Kh, _ = R.shape(ri, ro, quality)
    table = _rs(ri, ro, quality).host_table()
    hdr = table[:32].view(np.int32)
    assert len(table) == 32 + 4 * L * K
    assert hdr[0] == 0x50534552 and tuple(hdr[1:5]) == (L, M, K, Kh)
    assert tuple(hdr[5:8]) == (R.QUALITIES[quality][0], ri, ro)
    got = table[32:].view(np.float32).reshape(L, K)
    want = R.table(ri, ro, quality).astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def test_table_shapes_of_the_common_pairs():
    assert R.shape(44100, 22050)[:4] == (1, 2, 272, 136)
    assert R.shape(48000, 22050)[:4] == (147, 320, 296, 148)
    assert R.shape(16000, 22050)[:4] == (441, 320, 136, 68)
    assert R.shape(32000, 22050)[:4] == (441, 640, 198, 99)
    assert R.shape(44100, 16000)[:4] == (160, 441, 374, 187)


@pytest.mark.parametrize("ri,ro", R.PAIRS + ((32000, 22050),))
def test_output_lengths(ri, ro):
    L, M, _, _, _ = R.shape(ri, ro)
    rs = _rs(ri, ro, "fast")
    sizes = {0, 1, 2, 3, M - 1, M, M + 1, 7 * M - 1, 7 * M, 7 * M + 1, 66560, 133120, 2 ** 31 - 1}
    for j in (1, 2, 5):  # n_in L just below, on and just above a multiple of M
        sizes |= {(j * M) // L, (j * M) // L + 1, -(-(j * M) // L), max(0, (j * M) // L - 1)}
    for n_in in sorted(sizes):
        want = -((-n_in * L) // M)
        assert rs.n_out(n_in) == want == R.n_out(n_in, ri, ro), n_in


# ------------------------------------------------------------------------------- (f) refusals
def _cfg(**kw):
    from dcrecommend import _native as nat
    z, b, r = nat.RESAMPLE_QUALITIES["best"]
    v = dict(rate_in=44100, rate_out=22050, zeros=z, reserved=0, beta=b, rolloff=r)
    v.update(kw)
    return nat.ResampleConfig(*[v[f] for f, _ in nat.ResampleConfig._fields_])


BAD_CONFIGS = [(dict(rate_in=0), 1, "rate"), (dict(rate_out=0), 1, "rate"), (dict(rate_in=-44100), 1, "rate"),
               (dict(rate_in=22050), 1, "equal rates"), (dict(zeros=0), 1, "zeros"), (dict(zeros=-3), 1, "zeros"),
               (dict(rolloff=0.0), 1, "rolloff"), (dict(rolloff=1.0001), 1, "rolloff"), (dict(rolloff=-0.5), 1, "rolloff"),
               (dict(rolloff=float("nan")), 1, "rolloff"), (dict(beta=-1.0), 1, "beta"), (dict(beta=float("nan")), 1, "beta"),
               (dict(rate_in=44100, rate_out=44101), 2, "table"), (dict(rate_in=48000, rate_out=44101), 2, "table"),
               (dict(zeros=2 ** 31 - 1), 2, "table")]


@pytest.mark.parametrize("kw,status,word", BAD_CONFIGS)
def test_invalid_configurations_are_refused(kw, status, word):
    """DCUE_ERR_INVALID / DCUE_ERR_UNSUPPORTED with a dcue_last_error text from every entry point, with
    host memory and no launch."""
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg(**kw)
    n, b = ctypes.c_int64(), ctypes.c_size_t()
    buf = np.zeros(1 << 12, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    calls = [lambda: lib.dcue_resample_length(ctypes.byref(cfg), 1000, ctypes.byref(n)),
             lambda: lib.dcue_resample_table_bytes(ctypes.byref(cfg), ctypes.byref(b)),
             lambda: lib.dcue_resample_table_fill_host(ctypes.byref(cfg), p, buf.nbytes),
             lambda: lib.dcue_resample_table_init(ctypes.byref(cfg), p, buf.nbytes, None),
             lambda: lib.dcue_resample(ctypes.byref(cfg), p, p, 1, 1000, 0, 10, p, None)]
    launches = lib.dcue_launch_count()
    for call in calls:
        assert call() == status
        assert word in lib.dcue_last_error().decode()
    assert lib.dcue_launch_count() == launches


@pytest.mark.parametrize("n_clips,n_in,out0,n_out,status,word", [
    (-1, 1000, 0, 10, 1, "negative"), (1, -1, 0, 0, 1, "negative"), (1, 1000, -1, 10, 1, "negative"),
    (1, 1000, 0, -1, 1, "negative"),
    (1, 1000, 0, 501, 1, "output range"),    # 1000 samples at 2:1 give 500
    (1, 1000, 500, 1, 1, "output range"), (1, 1000, 1, 500, 1, "output range"), (1, 1001, 0, 502, 1, "output range"),
    (1, 0, 0, 1, 1, "output range"), (1, 1000, 2 ** 62, 2 ** 62, 1, "output range"),
    (1, 2 ** 31, 0, 10, 2, "2^31"),
])
def test_invalid_shapes_are_refused(n_clips, n_in, out0, n_out, status, word):
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg()
    buf = np.zeros(64, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    launches = lib.dcue_launch_count()
    assert lib.dcue_resample(ctypes.byref(cfg), p, p, n_clips, n_in, out0, n_out, p, None) == status
    assert word in lib.dcue_last_error().decode()
    assert lib.dcue_launch_count() == launches


def test_null_pointers_wrong_sizes_and_empty_calls():
    from dcrecommend import _native as nat
    lib, cfg = nat.lib(), _cfg()
    n, b = ctypes.c_int64(), ctypes.c_size_t()
    buf = np.zeros(4096, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    launches = lib.dcue_launch_count()
    assert lib.dcue_resample_table_bytes(ctypes.byref(cfg), ctypes.byref(b)) == 0 and b.value == 32 + 4 * 272
    for call, word in [
            (lambda: lib.dcue_resample_length(None, 10, ctypes.byref(n)), "null"),
            (lambda: lib.dcue_resample_length(ctypes.byref(cfg), 10, None), "null"),
            (lambda: lib.dcue_resample_table_bytes(None, ctypes.byref(b)), "null"),
            (lambda: lib.dcue_resample_table_bytes(ctypes.byref(cfg), None), "null"),
            (lambda: lib.dcue_resample_table_fill_host(None, p, b.value), "null"),
            (lambda: lib.dcue_resample_table_fill_host(ctypes.byref(cfg), None, b.value), "null"),
            (lambda: lib.dcue_resample_table_fill_host(ctypes.byref(cfg), p, b.value - 4), "table size"),
            (lambda: lib.dcue_resample_table_fill_host(ctypes.byref(cfg), p, b.value + 4), "table size"),
            (lambda: lib.dcue_resample_table_init(None, p, b.value, None), "null"),
            (lambda: lib.dcue_resample_table_init(ctypes.byref(cfg), None, b.value, None), "null"),
            (lambda: lib.dcue_resample_table_init(ctypes.byref(cfg), p, b.value - 4, None), "table size"),
            (lambda: lib.dcue_resample_table_init(ctypes.byref(_cfg(rate_in=48000)), p, b.value, None), "table size"),
            (lambda: lib.dcue_resample(None, p, p, 1, 1000, 0, 10, p, None), "null"),
            (lambda: lib.dcue_resample(ctypes.byref(cfg), None, p, 1, 1000, 0, 10, p, None), "null"),
            (lambda: lib.dcue_resample(ctypes.byref(cfg), p, None, 1, 1000, 0, 10, p, None), "null"),
            (lambda: lib.dcue_resample(ctypes.byref(cfg), p, p, 1, 1000, 0, 10, None, None), "null")]:
        assert call() == 1
        assert word in lib.dcue_last_error().decode(), word
    # nothing to do is DCUE_OK, whatever the pointers
    assert lib.dcue_resample(ctypes.byref(cfg), None, None, 0, 1000, 0, 10, None, None) == 0
    assert lib.dcue_resample(ctypes.byref(cfg), None, None, 3, 1000, 500, 0, None, None) == 0
    assert lib.dcue_launch_count() == launches


def test_python_front_end_validates_on_the_host():
    from dcrecommend import audio
    for args, word in (((0, 22050), "rate"), ((44100, 22050, "better"), "quality"), ((44100, 22050, (64, 14.7)), "quality"),
                       ((44100, 22050, (0, 14.7, 0.9)), "zeros"), ((44100, 22050, (64, -1.0, 0.9)), "beta"),
                       ((44100, 22050, (64, 14.7, 1.5)), "rolloff"), ((0, 0), "rate")):
        with pytest.raises(ValueError, match=word):
            audio.Resampler(*args)
    with pytest.raises(RuntimeError, match="table"):  # DCUE_ERR_UNSUPPORTED is not a ValueError
        audio.Resampler(44100, 44101)
    rs = audio.Resampler(44100, 22050, (16, 8.0, 0.8))
    assert rs.n_out(1001) == 501 and rs.quality == (16, 8.0, 0.8)
    same = audio.Resampler(22050, 22050)
    assert same.n_out(777) == 777
    with pytest.raises(ValueError, match="equal rates"):
        same.host_table()
    lm = audio.LogMel()
    assert lm.resampler(44100) is lm.resampler(44100) and lm.resampler(44100) is not lm.resampler(44100, "fast")
    assert lm.resampler(44100).rate_out == 22050


# ------------------------------------------------------------------------------------ (g) ABI
def test_abi_and_struct(tmp_path):
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == nat.ABI_VERSION
    assert nat.lib().dcue_abi_version() == 17
    for n in ("dcue_resample_length", "dcue_resample_table_bytes", "dcue_resample_table_fill_host",
              "dcue_resample_table_init", "dcue_resample"):
        assert re.search(r"^int %s\(" % n, hdr, flags=re.M), n
        assert n in nat._SIGS and hasattr(nat.lib(), n)
    assert "sample-rate conversion ahead of it (added under ABI 17)" in hdr
    assert eval(re.search(r"#define DCUE_RESAMPLE_MAX_TABLE_BYTES (\(.*\))", hdr).group(1)) == nat.RESAMPLE_MAX_TABLE_BYTES
    assert nat.RESAMPLE_QUALITIES == R.QUALITIES
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcue.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(dcue_resample_config));']
    for f, _ in nat.ResampleConfig._fields_:
        src.append('printf("%s %%zu\\n", offsetof(dcue_resample_config, %s));' % (f, f))
    src.append("return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.ResampleConfig) == 32
    for f, _ in nat.ResampleConfig._fields_:
        assert int(got[f]) == getattr(nat.ResampleConfig, f).offset, f


# ------------------------------------------------------------------------ (h) kernel resources
def test_resample_kernels_use_no_scratch(tmp_path):
    res = {k: v for k, v in kernel_resources("resample.hip", tmp_path).items() if "k_resample" in k}
    assert len(res) >= 1, sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 256, (name, r)
