"""fp64 numpy restatement of the audio front end (include/dcue.h, dcue_logmel): reflect pad, periodic
Hann window, |rfft|^2, Slaney mel filterbank (linear below 1 kHz, logarithmic above, triangles with
area normalisation 2 / (f[i+2] - f[i]) -- librosa's defaults, written here from the formulas), and the
three compressions. The reference project has no code for this step (its transform_audio.py was never
published), so this file is the contract the kernel is held to.

Also the input generators the tests share, and the float32 CPU route through torch.stft that the
tolerances are measured against."""
import math

import numpy as np

N_MELS = 128
POWER, DB, LOG1P = 0, 1, 2

# Measured f32 distances: the largest distance of torch's float32 CPU route (torch.stft, center=True,
# pad_mode="reflect", then the filterbank product in float32) from this fp64 oracle over every parity
# input of tests/test_logmel_cpu.py (all n_fft x hop x n_samples of the GPU grid, every generator).
#   D_LIN: max over frames of max_bin |P32 - P64| / max_bin P64 (mel power)
#   D_DB : max |dB32 - dB64| over the noise-floored inputs at amin = parity_amin(n_fft) (dynamic range
#          of the oracle's dB output < 80 dB), in dB
#   D_L1P: max |l32 - l64| of log(1 + 10 sqrt(P)) over the same inputs
# Measured 2026-10-20 with `pytest tests/test_logmel_cpu.py -k oracle_against_torch -s`, which prints
# the three figures and asserts that they are within a factor of two of these constants.
D_LIN = 5.32e-7
D_DB = 4.81e-4
D_L1P = 3.28e-6


def n_frames(n_samples, n_fft, hop, center=True):
    pad = n_fft // 2 if center else 0
    return 1 + (n_samples + 2 * pad - n_fft) // hop


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


def _hz_to_mel(f):
    f_sp = 200.0 / 3.0
    if f < 1000.0:
        return f / f_sp
    return 1000.0 / f_sp + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _mel_to_hz(m):
    f_sp = 200.0 / 3.0
    min_log_mel = 1000.0 / f_sp
    if m < min_log_mel:
        return f_sp * m
    return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - min_log_mel))


def mel_points(fmin, fmax):
    """The 130 band edges in Hz: equally spaced on the Slaney mel scale from fmin to fmax."""
    m0, m1 = _hz_to_mel(float(fmin)), _hz_to_mel(float(fmax))
    step = (m1 - m0) / (N_MELS + 1)
    return np.array([_mel_to_hz(m0 + i * step) for i in range(N_MELS + 2)], dtype=np.float64)


def filterbank(sample_rate, n_fft, fmin=0.0, fmax=None):
    """[128][n_fft/2 + 1] fp64 weights."""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    f = mel_points(fmin, fmax)
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * float(sample_rate) / n_fft
    fb = np.zeros((N_MELS, n_fft // 2 + 1), dtype=np.float64)
    for i in range(N_MELS):
        lower = (freqs - f[i]) / (f[i + 1] - f[i])
        upper = (f[i + 2] - freqs) / (f[i + 2] - f[i + 1])
        fb[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[i + 2] - f[i]))
    return fb


def filter_ranges(fb):
    """(first [128], count [128], packed weights) of the nonzero run of each filter; an empty filter
    has first 0 and count 0."""
    first = np.zeros(N_MELS, dtype=np.int32)
    count = np.zeros(N_MELS, dtype=np.int32)
    packed = []
    for i in range(N_MELS):
        nz = np.nonzero(fb[i] > 0.0)[0]
        if len(nz):
            assert nz[-1] - nz[0] + 1 == len(nz)  # a triangle is one contiguous run
            first[i], count[i] = nz[0], len(nz)
            packed.append(fb[i, nz[0]:nz[-1] + 1])
    return first, count, (np.concatenate(packed) if packed else np.zeros(0))


def frames(wave, n_fft, hop, center=True):
    """[n][T][n_fft] fp64 frames of [n][n_samples], reflect-padded by n_fft/2 when center."""
    x = np.asarray(wave, dtype=np.float64)
    if center:
        x = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    T = 1 + (x.shape[1] - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return x[:, idx]


def mel_power(wave, sample_rate=22050, n_fft=1024, hop=512, fmin=0.0, fmax=None, center=True):
    """[n][T][128] fp64 mel power."""
    fr = frames(wave, n_fft, hop, center) * hann(n_fft)
    spec = np.abs(np.fft.rfft(fr, axis=-1)) ** 2
    return spec @ filterbank(sample_rate, n_fft, fmin, fmax).T


def compress(P, mode, amin=1e-10, log_scale=10.0, top_db=None):
    if mode == POWER:
        return P
    if mode == DB:
        out = 10.0 * np.log10(np.maximum(P, amin))
        if top_db is not None:
            out = np.maximum(out, out.max(axis=(1, 2), keepdims=True) - top_db)
        return out
    if mode == LOG1P:
        return np.log1p(log_scale * np.sqrt(P))
    raise ValueError(mode)


def logmel(wave, mode=DB, amin=1e-10, log_scale=10.0, top_db=None, **kw):
    return compress(mel_power(wave, **kw), mode, amin, log_scale, top_db)


def dynamic_range_db(P, amin=0.0):
    """Largest over clips of 10 log10(max P / max(min P, amin)): the span of the clip's dB output."""
    P = np.maximum(P.reshape(P.shape[0], -1), amin)
    return float(np.max(10.0 * np.log10(P.max(axis=1) / P.min(axis=1))))


def parity_amin(n_fft):
    """The dB floor of the dB parity cases. A frame centred on the clip's first or last sample is
    even-symmetric, so a spectrum bin of it is one real number that can pass through zero, and at n_fft
    256 / 512 many mel filters are a single FFT bin: with the default amin = 1e-10 such inputs span far
    more than 80 dB whatever their noise floor, and no float32 route resolves those bins. The floor sits
    80 dB below 100 (n_fft / 256)^2, above the largest mel power of the parity inputs (peak power grows
    with n_fft^2), so the oracle's dB output spans less than 80 dB -- which the tests assert."""
    return 1e-6 * (n_fft / 256.0) ** 2


def frame_distance(got, want):
    """max over frames of max_bin |got - want| / max_bin want (frames of silence: absolute)."""
    num = np.abs(np.asarray(got, dtype=np.float64) - want).max(axis=-1)
    den = want.max(axis=-1)
    return float(np.max(num / np.where(den > 0.0, den, 1.0)))


# ------------------------------------------------------------------------------------ inputs
def white_noise(n, n_samples, seed=0):
    return (0.1 * np.random.RandomState(seed).standard_normal((n, n_samples))).astype(np.float32)


def tones(n, n_samples, sample_rate=22050, seed=1, floor=0.05):
    """Three sines per clip plus a white noise floor (floor = 0: pure tones)."""
    rng = np.random.RandomState(seed)
    t = np.arange(n_samples, dtype=np.float64) / sample_rate
    out = np.zeros((n, n_samples))
    for c in range(n):
        for _ in range(3):
            out[c] += rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(60.0, 9000.0) * t + rng.uniform(0, 6.28))
    return (out + floor * rng.standard_normal((n, n_samples))).astype(np.float32)


def chirp(n, n_samples, sample_rate=22050, seed=2, floor=0.05):
    """A linear sweep per clip plus a white noise floor."""
    rng = np.random.RandomState(seed)
    t = np.arange(n_samples, dtype=np.float64) / sample_rate
    dur = max(n_samples / sample_rate, 1e-9)
    out = np.zeros((n, n_samples))
    for c in range(n):
        f0, f1 = rng.uniform(50.0, 500.0), rng.uniform(3000.0, 10000.0)
        out[c] = 0.25 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t))
    return (out + floor * rng.standard_normal((n, n_samples))).astype(np.float32)


def impulses(n, n_samples):
    """Unit impulses at sample 0, sample 1 and the last sample, cycling over the clips."""
    out = np.zeros((n, n_samples), dtype=np.float32)
    for c in range(n):
        out[c, (0, 1, n_samples - 1)[c % 3]] = 1.0
    return out


def silence(n, n_samples):
    return np.zeros((n, n_samples), dtype=np.float32)


LINEAR_INPUTS = ("white_noise", "tones", "pure_tones", "chirp", "impulses", "silence")
FLOORED_INPUTS = ("white_noise", "tones", "chirp")  # dynamic range below 80 dB: the dB / log1p inputs


def make_input(name, n, n_samples, sample_rate=22050):
    if name == "white_noise":
        return white_noise(n, n_samples)
    if name == "tones":
        return tones(n, n_samples, sample_rate)
    if name == "pure_tones":
        return tones(n, n_samples, sample_rate, floor=0.0)
    if name == "chirp":
        return chirp(n, n_samples, sample_rate)
    if name == "impulses":
        return impulses(n, n_samples)
    if name == "silence":
        return silence(n, n_samples)
    raise KeyError(name)


def torch_route(wave, sample_rate=22050, n_fft=1024, hop=512, fmin=0.0, fmax=None):
    """The independent float32 route: torch.stft on the CPU, then the filterbank product, [n][T][128]."""
    import torch
    x = torch.as_tensor(np.asarray(wave, dtype=np.float32))
    # the window rounded once from fp64, as the library's table holds it: torch.hann_window in float32
    # loses its relative accuracy at the window's edges, which an impulse next to an edge would show
    win = torch.as_tensor(hann(n_fft).astype(np.float32))
    s = torch.stft(x, n_fft, hop_length=hop, window=win, center=True, pad_mode="reflect", return_complex=True)
    p = s.real ** 2 + s.imag ** 2  # [n][bins][T]
    fb = torch.as_tensor(filterbank(sample_rate, n_fft, fmin, fmax).astype(np.float32))
    return torch.matmul(fb, p).transpose(1, 2).contiguous().numpy()
