"""The augmentation rule of include/dcue.h (dcue_crop_tracks_augmented) restated in Python integers and
numpy fp32 / fp16, from the header's text alone: it never calls the library. The tests compare the
library with it bit for bit (NaNs as NaNs).

    h = crop_hash(seed, draw, t) whatever the mode;  r(i) = mix(h + G (i + 1))
    gain          u24 = r(0) >> 40,  g = gain_db * (float32(u24) * 2^-23 - 1)
    freq mask j   w = (r(1 + 2j) * (F + 1)) >> 64,  p = (r(2 + 2j) * (128 - w + 1)) >> 64:  bins [p, p + w)
    time mask j   w = min((r(9 + 2j) * (T + 1)) >> 64, n),  p = (r(10 + 2j) * (n - w + 1)) >> 64:  frames [p, p + w)
    element       masked: fill; else x + g (fp32; no add with gain_db == 0); then the cast to out_dtype
    fill          CONST: fill_value.  MEAN: m + g (m with gain_db == 0), m = float32(float64(S) * 2^-24 / (n * 128)),
                  S the exact sum of the valid elements rounded to fp16, in units of 2^-24; NaN if one is not finite
"""
import numpy as np

import crop_reference as R

MAX_MASKS = 4
FILL_MEAN, FILL_CONST = 0, 1


class Aug:
    """One configuration; fill is 'mean' or the constant."""

    def __init__(self, n_freq=0, freq_width=0, n_time=0, time_width=0, gain_db=0.0, fill="mean"):
        self.n_freq, self.freq_width, self.n_time, self.time_width = n_freq, freq_width, n_time, time_width
        self.gain_db, self.fill = np.float32(gain_db), fill

    def off(self):
        return self.n_freq * self.freq_width == 0 and self.n_time * self.time_width == 0 and self.gain_db == 0

    def key(self):
        return (self.n_freq, self.freq_width, self.n_time, self.time_width, float(self.gain_db), self.fill)


def r(h, i):
    return R.mix((h + R.G * (i + 1)) & R.MASK)


def params(aug, seed, draw, t, L):
    """(g float32, [(p, w)] * n_freq, [(p, w)] * n_time) of the track at store index t with L frames."""
    h = R.crop_hash(seed, draw, int(t))
    n = min(int(L), R.W)
    u24 = r(h, 0) >> 40
    c = np.float32(u24) * np.float32(2.0 ** -23) - np.float32(1.0)  # both exact
    g = np.float32(aug.gain_db) * np.float32(c)
    freq, time = [], []
    for j in range(aug.n_freq):
        w = (r(h, 1 + 2 * j) * (aug.freq_width + 1)) >> 64
        freq.append(((r(h, 2 + 2 * j) * (R.N_MELS - w + 1)) >> 64, w))
    for j in range(aug.n_time):
        w = min((r(h, 1 + 2 * MAX_MASKS + 2 * j) * (aug.time_width + 1)) >> 64, n)
        time.append(((r(h, 2 + 2 * MAX_MASKS + 2 * j) * (n - w + 1)) >> 64, w))
    return np.float32(g), freq, time


def exact_mean(x16):
    """float32 mean of an fp16 array by the header's rule: the exact sum in units of 2^-24 as a Python
    integer, one rounding to float64, the scaling (exact), one division, one rounding to float32."""
    if not np.all(np.isfinite(x16)):
        return np.float32(np.nan)
    units = x16.astype(np.float64) * 2.0 ** 24  # exact: integers below 2^41
    assert np.array_equal(units, np.rint(units))
    S = int(units.astype(np.int64).sum())  # at most 16,768 of them: below 2^55, no wrap
    return np.float32(np.float64(float(S)) * np.float64(2.0 ** -24) / np.float64(x16.size))


def mask(aug, freq, time, n):
    """bool [n][128]: the union of the masks over the n valid frames."""
    m = np.zeros((n, R.N_MELS), dtype=bool)
    for p, w in freq:
        m[:, p:p + w] = True
    for p, w in time:
        m[p:p + w, :] = True
    return m


def crop(data, frame_ptr, rows, out_dtype, aug, mode=R.RANDOM, total_frames=None, **kw):
    """(out, starts, flags) of dcue_crop_tracks_augmented: crop_reference.crop's windows, augmented."""
    n_tracks = len(frame_ptr) - 1
    total = len(data) if total_frames is None else total_frames
    rows = np.arange(n_tracks) if rows is None else np.asarray(rows)
    seed, draw = kw.get("seed", 0), kw.get("draw", 0)
    out = np.zeros((len(rows), R.W, R.N_MELS), dtype=out_dtype)
    st = np.zeros(len(rows), dtype=np.int32)
    flags = np.zeros(len(rows), dtype=np.int32)
    done = {}
    for i, t in enumerate(rows):
        t = int(t)
        if t < 0 or t >= n_tracks:
            flags[i] = R.FLAG_BAD_ROW
            continue
        lo, hi = int(frame_ptr[t]), int(frame_ptr[t + 1])
        if lo < 0 or hi < lo or hi > total:
            flags[i] = R.FLAG_BAD_EXTENT
            continue
        if t not in done:
            L = hi - lo
            s = R.start(mode, L, t, **kw)
            n = min(L, R.W)
            src = data[lo + s:lo + s + n]
            g, freq, time = params(aug, seed, draw, t, L)
            gain_on = aug.gain_db != 0
            if aug.off():
                row = src.astype(out_dtype)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    row = (src.astype(np.float32) + g).astype(out_dtype) if gain_on else src.astype(out_dtype)
                    m = mask(aug, freq, time, n)
                    if m.any():
                        if aug.fill == "mean":
                            fill = exact_mean(src.astype(np.float16))
                            if gain_on:
                                fill = np.float32(fill + g)
                        else:
                            fill = np.float32(aug.fill)
                        row[m] = np.float32(fill).astype(out_dtype)
            done[t] = (row, s)
        row, s = done[t]
        out[i, :len(row)] = row
        st[i] = s
    return out, st, flags


# the cases the GPU test's setup must contain, as the issue counted them over the 37-track store
CASE_AUG = dict(n_freq=2, freq_width=27, n_time=2, time_width=40)
CASE_PAIRS = ((0, 0), (7, 2 ** 40), (0, 1), (3, 5))
CASE_COUNTS = {"freq width 0": 11, "freq at bin 0": 2, "freq ends at bin 128": 6, "two freq masks overlap": 30,
               "time width 0 on a non-empty track": 5, "time mask clipped by a short track": 32,
               "time mask covers the last valid frame of a longer track": 3, "time mask covers every valid frame": 32}


def case_counts(lengths, aug, pairs=CASE_PAIRS):
    """How often each case of CASE_COUNTS occurs over tracks of `lengths` at the (seed, draw) pairs, and
    whether gains of both signs occur."""
    c = dict.fromkeys(CASE_COUNTS, 0)
    signs = set()
    for seed, draw in pairs:
        for t, L in enumerate(lengths):
            L = int(L)
            n = min(L, R.W)
            g, freq, time = params(aug, seed, draw, t, L)
            signs.add(bool(g > 0) - bool(g < 0))
            h = R.crop_hash(seed, draw, t)
            for p, w in freq:
                c["freq width 0"] += w == 0
                c["freq at bin 0"] += p == 0 and w > 0
                c["freq ends at bin 128"] += p + w == R.N_MELS and w > 0
            (p0, w0), (p1, w1) = freq[:2]
            c["two freq masks overlap"] += w0 > 0 and w1 > 0 and p0 < p1 + w1 and p1 < p0 + w0
            for j, (p, w) in enumerate(time):
                drawn = (r(h, 1 + 2 * MAX_MASKS + 2 * j) * (aug.time_width + 1)) >> 64  # before the clip to n
                c["time width 0 on a non-empty track"] += w == 0 and L > 0
                c["time mask clipped by a short track"] += drawn > n and L in (1, 130)
                c["time mask covers the last valid frame of a longer track"] += 0 < w < n and p + w == n
                c["time mask covers every valid frame"] += w == n and n > 0
    return c, signs
