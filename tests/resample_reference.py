"""fp64 numpy restatement of the sample-rate conversion (include/dcue.h, dcue_resample): a rational
polyphase resampler with a Kaiser-windowed sinc evaluated exactly per phase. The reference project has no
code for this step, so this file is the contract the kernel is held to; tests/test_resample_cpu.py checks
it against scipy.signal.resample_poly, an independent implementation of the same filter.

Also the float32 CPU route through torch.conv1d that the GPU tolerance is measured against. The input
generators are logmel_reference's."""
import math

import numpy as np

from logmel_reference import LINEAR_INPUTS, make_input  # noqa: F401  (shared with the GPU tests)

# (zeros, beta, rolloff): the published constants of resampy's kaiser_best / kaiser_fast windows
QUALITIES = {"best": (64, 14.769656459379492, 0.9475937167399596), "fast": (16, 8.555504641634386, 0.85)}
PAIRS = ((44100, 22050), (22050, 44100), (48000, 22050), (16000, 22050), (44100, 16000))

# Measured f32 distance: the largest, over every clip of the GPU parity grid (PAIRS x QUALITIES x
# parity_sizes x every generator, tests/test_resample_cpu.py), of max_m |y32 - y64| / max_m |y64| (absolute
# for a clip of silence) of the float32 CPU route (torch_route below) from this fp64 oracle.
# Measured 2026-10-20 with `pytest tests/test_resample_cpu.py -k f32_distance -s`, which prints the figure
# and asserts that it is within a factor of two of this constant.
D_RS = 1.26e-6

# What the two fp64 oracles (this resampler, then logmel_reference.mel_power) give for the layer test's
# 1 kHz + 3 kHz pair: frame_distance of the mel power of the 44,100 Hz clip resampled to 22,050 Hz (best)
# from the mel power of the same tones generated at 22,050 Hz, over the frames that do not touch the
# clip's ends. Printed and held within a factor of two by test_resample_cpu.py -k tone_pair.
D_TONE_PAIR = 1.5e-8


def shape(rate_in, rate_out, quality="best"):
    """(L, M, K, Kh, s) of a rate pair."""
    zeros, _, rolloff = QUALITIES[quality] if isinstance(quality, str) else quality
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    s = rolloff * (L / M if L < M else 1.0)
    Kh = int(math.ceil(zeros / s))
    return L, M, 2 * Kh, Kh, s


def n_out(n_in, rate_in, rate_out):
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    return -((-int(n_in) * L) // M)


def table(rate_in, rate_out, quality="best"):
    """[L][K] fp64 taps: tab[p][k] = s sinc(u) w(u), u = s (p / L - (k - Kh + 1))."""
    zeros, beta, _ = QUALITIES[quality] if isinstance(quality, str) else quality
    L, M, K, Kh, s = shape(rate_in, rate_out, quality)
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    u = s * (p / L - (k - Kh + 1))
    pu = np.pi * u
    sinc = np.where(u == 0.0, 1.0, np.sin(pu) / np.where(u == 0.0, 1.0, pu))
    r = u / zeros
    w = np.where(np.abs(u) < zeros, np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(beta), 0.0)
    return s * sinc * w


def resample(wave, rate_in, rate_out, quality="best", out0=0, count=None):
    """[n][count] fp64: outputs out0 .. out0 + count - 1 (default: to the end) of each clip of [n][n_in]."""
    x = np.atleast_2d(np.asarray(wave, dtype=np.float64))
    L, M, K, Kh, _ = shape(rate_in, rate_out, quality)
    tab = table(rate_in, rate_out, quality)
    n_in = x.shape[1]
    total = n_out(n_in, rate_in, rate_out)
    count = total - out0 if count is None else count
    assert 0 <= out0 and out0 + count <= total
    m = out0 + np.arange(count, dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    y = np.zeros((x.shape[0], count), dtype=np.float64)
    for lo in range(0, count, 4096):  # bounded memory: [rows][K] index blocks
        hi = min(count, lo + 4096)
        idx = q[lo:hi, None] - Kh + 1 + np.arange(K, dtype=np.int64)[None, :]
        ok = (idx >= 0) & (idx < n_in)
        w = tab[p[lo:hi]] * ok
        y[:, lo:hi] = np.einsum("ck,nck->nc", w, x[:, np.where(ok, idx, 0)])
    return y


def upsampled_fir(rate_in, rate_out, quality="best"):
    """The same taps on the upsampled grid, for scipy.signal.resample_poly(x, L, M, window=hu) / L:
    hu[p - L (k - Kh + 1) + L Kh] = tab[p][k], length 2 L Kh + 1 (odd: the centre is index L Kh)."""
    L, M, K, Kh, _ = shape(rate_in, rate_out, quality)
    tab = table(rate_in, rate_out, quality)
    hu = np.zeros(2 * L * Kh + 1, dtype=np.float64)
    p = np.arange(L)[:, None]
    k = np.arange(K)[None, :]
    hu[p - L * (k - Kh + 1) + L * Kh] = tab
    return hu


def conv_weight(rate_in, rate_out, quality="best"):
    """The phase filters as one conv1d weight of stride M, as torchaudio formulates resampling: output
    L j + i of a clip is channel i at position j. Row i is phase row (i M) mod L shifted right by
    floor(i M / L) samples, zero elsewhere; the clip is zero-padded by Kh - 1 in front. [L][W] fp64."""
    L, M, K, Kh, _ = shape(rate_in, rate_out, quality)
    tab = table(rate_in, rate_out, quality)
    W = K + ((L - 1) * M) // L
    w = np.zeros((L, W), dtype=np.float64)
    for i in range(L):
        w[i, (i * M) // L:(i * M) // L + K] = tab[(i * M) % L]
    return w


def torch_route(wave, rate_in, rate_out, quality="best", device="cpu"):
    """The float32 route: torch.conv1d over the phase filters with stride M. [n][n_out] float32 tensor."""
    import torch
    x = torch.as_tensor(np.atleast_2d(np.asarray(wave, dtype=np.float32))).to(device)
    L, M, K, Kh, _ = shape(rate_in, rate_out, quality)
    w = torch.as_tensor(conv_weight(rate_in, rate_out, quality).astype(np.float32)).to(device)
    return conv_route(x, w, L, M, Kh)


def conv_route(x, w, L, M, Kh):
    """x [n][n_in] and w [L][W] float32 tensors on one device -> [n][ceil(n_in L / M)]."""
    import torch
    n, n_in = x.shape
    total = -((-n_in * L) // M)
    blocks = -(-total // L)
    need = (blocks - 1) * M + w.shape[1]  # samples the last block's window ends at
    xp = torch.nn.functional.pad(x, (Kh - 1, max(0, need - (Kh - 1) - n_in)))
    y = torch.nn.functional.conv1d(xp[:, None, :], w[:, None, :], stride=M)  # [n][L][blocks]
    return y.transpose(1, 2).reshape(n, -1)[:, :total].contiguous()


def clip_distance(got, want):
    """Per clip: max_m |got - want| / max_m |want| (a clip of silence: absolute). [n] fp64."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape[1] == 0:
        return np.zeros(got.shape[0])
    den = np.abs(want).max(axis=1)
    return np.abs(got - want).max(axis=1) / np.where(den > 0.0, den, 1.0)


def parity_sizes(rate_in, rate_out, quality):
    """n_in of the GPU parity grid: 1, Kh - 1, K + 1 and 4097."""
    _, _, K, Kh, _ = shape(rate_in, rate_out, quality)
    return (1, Kh - 1, K + 1, 4097)


def batch(n_samples, sample_rate):
    """37 clips cycling through every generator (clip c: generator c % 6, its row c // 6, so the three
    impulse positions all occur), and each clip's generator name."""
    names = [LINEAR_INPUTS[c % len(LINEAR_INPUTS)] for c in range(37)]
    rows = {name: make_input(name, 7, n_samples, sample_rate) for name in LINEAR_INPUTS if name != "impulses"}
    rows["impulses"] = np.zeros((7, n_samples), dtype=np.float32)
    for c in range(7):  # logmel_reference.impulses, for clips as short as one sample
        rows["impulses"][c, min((0, 1, n_samples - 1)[c % 3], n_samples - 1)] = 1.0
    x = np.stack([rows[names[c]][c // len(LINEAR_INPUTS)] for c in range(37)])
    return x, names


def tone_pair(n_samples, sample_rate):
    """1 kHz + 3 kHz, float32, n_samples at sample_rate."""
    t = np.arange(n_samples, dtype=np.float64) / sample_rate
    return (0.3 * np.sin(2 * np.pi * 1000.0 * t) + 0.2 * np.sin(2 * np.pi * 3000.0 * t)).astype(np.float32)[None, :]
