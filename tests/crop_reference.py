"""The window rule of include/dcue.h (dcue_crop_tracks) restated in numpy / Python integers, from the
header's text alone: it never calls the library. The tests compare the library with it bit for bit.

    L <= W:   start 0, the L frames copied, the other W - L rows zero
    FIRST:    0            CENTER: (L - W) // 2
    GRID:     grid_j * (L - W) // (grid_n - 1); grid_n == 1 is CENTER
    RANDOM:   (h * (L - W)) >> 64, h = mix(mix(seed + G (t + 1)) + G (draw + 1)) modulo 2^64
"""
import numpy as np

W = 131
N_MELS = 128
FIRST, CENTER, GRID, RANDOM = 0, 1, 2, 3
FLAG_BAD_EXTENT, FLAG_BAD_ROW = 1, 2
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
FACTOR_DRAW0 = 1 << 32

# the lengths every test draws from: empty, one frame, one short of / exactly / one and two past a
# window, two windows, config 2's previews
LENGTHS = (0, 1, 130, 131, 132, 133, 262, 1292)


def mix(z):
    """The splitmix64 finaliser."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def crop_hash(seed, draw, t):
    z0 = mix((seed + G * (t + 1)) & MASK)
    return mix((z0 + G * (draw + 1)) & MASK)


def start(mode, L, t, seed=0, draw=0, grid_j=0, grid_n=1):
    span = int(L) - W
    if span <= 0 or mode == FIRST:
        return 0
    if mode == CENTER or (mode == GRID and grid_n == 1):
        return span // 2
    if mode == GRID:
        return grid_j * span // (grid_n - 1)
    if mode == RANDOM:
        return (crop_hash(seed, draw, int(t)) * span) >> 64
    raise ValueError(mode)


def starts(mode, lengths, track_ids=None, **kw):
    ids = range(len(lengths)) if track_ids is None else track_ids
    return np.array([start(mode, L, t, **kw) for L, t in zip(lengths, ids)], dtype=np.int64)


def mix_np(z):
    """mix over a uint64 array (wrapping arithmetic)."""
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def random_starts_np(span, seed, draws, ts):
    """RANDOM starts for one span < 2^32 over arrays of draws and track indices (vectorised: the high
    64 bits of h * span from the two 32-bit halves of h)."""
    with np.errstate(over="ignore"):
        g = np.uint64(G)
        z0 = mix_np(np.uint64(seed) + g * (np.asarray(ts, dtype=np.uint64) + np.uint64(1)))
        h = mix_np(z0 + g * (np.asarray(draws, dtype=np.uint64) + np.uint64(1)))
        s = np.uint64(span)
        lo, hi = h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)
        return ((hi * s + ((lo * s) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def make_store(lengths, dtype, seed=0):
    """(data [total][128] of dtype, frame_ptr int64 [n + 1]): random values, every one exactly
    representable in fp16 when dtype is float16; fp32 stores hold values that are not (so the
    conversion to fp16 has something to round), with ties to even among them."""
    rs = np.random.RandomState(seed)
    total = int(np.sum(lengths))
    x = rs.randn(total, N_MELS).astype(np.float32)
    if total:
        x[0, :4] = [1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 65519.0]  # ties, the largest finite
    frame_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return x.astype(dtype), frame_ptr


def crop(data, frame_ptr, rows, out_dtype, mode, total_frames=None, **kw):
    """(out [n][131][128] of out_dtype, starts int32 [n], flags int32 [n]) as the header defines them.
    rows None: track i. numpy's float32 -> float16 cast rounds to nearest even."""
    n_tracks = len(frame_ptr) - 1
    total = len(data) if total_frames is None else total_frames
    rows = np.arange(n_tracks) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), W, N_MELS), dtype=out_dtype)
    st = np.zeros(len(rows), dtype=np.int32)
    flags = np.zeros(len(rows), dtype=np.int32)
    for i, t in enumerate(rows):
        t = int(t)
        if t < 0 or t >= n_tracks:
            flags[i] = FLAG_BAD_ROW
            continue
        lo, hi = int(frame_ptr[t]), int(frame_ptr[t + 1])
        if lo < 0 or hi < lo or hi > total:
            flags[i] = FLAG_BAD_EXTENT
            continue
        L = hi - lo
        s = start(mode, L, t, **kw)
        n = min(L, W)
        out[i, :n] = data[lo + s:lo + s + n].astype(out_dtype)
        st[i] = s
    return out, st, flags
