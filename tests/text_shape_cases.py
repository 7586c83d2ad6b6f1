"""The shapes tests/test_gpu_text_shapes.py runs against the fp64 oracle, and the variant keys of the
text branch's launches (dcue_debug_text_shape). tests/test_text_shapes_cpu.py asserts that these
cases reach every key a shape can select, so a threshold of launch_text_fwd / launch_text_wgrad that
moves must bring a case along. No GPU is touched at import."""
import ctypes

TEXT = "truedcuemel1dbntext"
PAD = 0

# (layout, B, N, T, text_dim, word_dim, n_words). Catalogue: M = B (1 + N); in-batch: M = B.
CASES = [
    # full TBW 1, 4 waves, BPD 3 over one K chunk, E < 32, nxcd 4 with an idle XCD, Creal < C_s
    ("catalogue", 1, 2, 2, 40, 4, 60),
    # TBW 2 ragged, 8 waves, BPD 6 = all six steps; wgrad: one pass of 17..32 items
    ("catalogue", 3, 5, 17, 100, 64, 60),
    # TBW 4 ragged, odd chunk count (BPD 3); one pass of 33..48 items
    ("inbatch", 40, 20, 33, 64, 96, 60),
    # config 4's kernel (NCH 10), two column blocks, 130 units on 8 XCDs with a tail, a second
    # staging pass of one item, E % 32 != 0
    ("catalogue", 13, 4, 64, 256, 300, 500),
    # TBW 8, two wgrad chunks (65 + 64) + reduce, positions up to 127
    ("catalogue", 43, 2, 128, 40, 100, 60),
    # chunked <8,1> through the LDS limit, two chunks
    ("catalogue", 13, 9, 128, 256, 300, 500),
    # chunked <4,2>, half-empty last workgroup, 18 word blocks
    ("catalogue", 1, 6, 64, 64, 576, 60),
    # three full chunks of two full passes
    ("catalogue", 128, 2, 32, 128, 128, 60),
    # the 16-chunk cap: 130 items per chunk (64 + 64 + 2), last chunk 115
    ("catalogue", 295, 6, 16, 64, 32, 60),
]

# Added until test_text_shapes_cpu.py's closure passed, the smallest M that selects each: every
# (TBW, waves, BPD, NCH) instantiation with an even and a ragged unit count on four XCDs (M = 4 / 3)
# and on eight (M >= 129, or 65 at two column blocks), the full <4,2> workgroup, and the remaining
# (chunks, passes, last pass) classes of the weight gradient. The comment names the keys a case alone
# covers: the forward's (kernel, TBW, waves, BPD, NCH > 0, nxcd, ragged), then the weight gradient's.
CASES += [
    ("catalogue", 1, 2, 3, 40, 292, 60),  # ('full', 1, 4, 6, True, 4, True)
    ("catalogue", 1, 2, 3, 128, 1024, 60),  # ('full', 1, 8, 6, False, 4, True)
    ("catalogue", 1, 2, 9, 100, 320, 60),  # ('full', 1, 8, 6, True, 4, True)
    ("catalogue", 1, 2, 16, 64, 548, 60),  # ('full', 1, 4, 6, False, 4, True)
    ("catalogue", 1, 2, 16, 100, 68, 60),  # ('full', 1, 8, 3, False, 4, True)
    ("catalogue", 1, 2, 17, 40, 4, 60),  # ('full', 2, 4, 3, False, 4, True)
    ("catalogue", 1, 2, 17, 40, 292, 60),  # ('full', 2, 4, 6, True, 4, True)
    ("catalogue", 1, 2, 25, 64, 548, 60),  # ('full', 2, 4, 6, False, 4, True)
    ("catalogue", 1, 2, 25, 100, 300, 60),  # ('full', 2, 8, 6, True, 4, True)
    ("catalogue", 1, 2, 33, 40, 292, 60),  # ('full', 4, 4, 6, True, 4, True)
    ("catalogue", 1, 2, 33, 100, 288, 60),  # ('full', 4, 8, 3, False, 4, True)
    ("catalogue", 1, 2, 48, 100, 36, 60),  # ('full', 4, 8, 6, False, 4, True)
    ("catalogue", 1, 2, 64, 64, 32, 60),  # ('full', 4, 4, 3, False, 4, True)
    ("catalogue", 1, 2, 64, 64, 36, 60),  # ('full', 4, 4, 6, False, 4, True)
    ("catalogue", 1, 2, 64, 128, 292, 60),  # ('full', 4, 8, 6, True, 4, True)
    ("catalogue", 1, 2, 100, 256, 288, 60),  # ('full', 8, 8, 3, False, 4, True)
    ("catalogue", 2, 1, 2, 256, 548, 60),  # ('full', 1, 8, 6, False, 4, False)
    ("catalogue", 2, 1, 3, 256, 8, 60),  # ('full', 1, 8, 3, False, 4, False)
    ("catalogue", 2, 1, 16, 40, 96, 60),  # ('full', 1, 4, 3, False, 4, False)
    ("catalogue", 2, 1, 16, 40, 128, 60),  # ('full', 1, 4, 6, False, 4, False)
    ("catalogue", 2, 1, 16, 64, 300, 60),  # ('full', 1, 4, 6, True, 4, False)
    ("catalogue", 2, 1, 16, 128, 300, 60),  # ('full', 1, 8, 6, True, 4, False)
    ("catalogue", 2, 1, 17, 100, 32, 60),  # ('full', 2, 8, 3, False, 4, False)
    ("catalogue", 2, 1, 25, 40, 8, 60),  # ('full', 2, 4, 3, False, 4, False)
    ("catalogue", 2, 1, 25, 64, 320, 60),  # ('full', 2, 4, 6, True, 4, False)
    ("catalogue", 2, 1, 25, 100, 36, 60),  # ('full', 2, 8, 6, False, 4, False)
    ("catalogue", 2, 1, 25, 256, 320, 60),  # ('full', 2, 8, 6, True, 4, False)
    ("catalogue", 2, 1, 32, 64, 1024, 60),  # ('full', 2, 4, 6, False, 4, False)
    ("catalogue", 2, 1, 33, 64, 292, 60),  # ('full', 4, 4, 6, True, 4, False)
    ("catalogue", 2, 1, 48, 40, 576, 60),  # ('chunked', 4, 2, 0, False, 0, False)
    ("catalogue", 2, 1, 48, 64, 128, 60),  # ('full', 4, 4, 6, False, 4, False)
    ("catalogue", 2, 1, 48, 100, 320, 60),  # ('full', 4, 8, 6, True, 4, False)
    ("catalogue", 2, 1, 64, 100, 68, 60),  # ('full', 4, 8, 3, False, 4, False)
    ("catalogue", 2, 1, 64, 128, 100, 60),  # ('full', 4, 8, 6, False, 4, False)
    ("catalogue", 2, 1, 65, 64, 256, 60),  # ('full', 8, 4, 3, False, 4, False)
    ("catalogue", 2, 1, 65, 256, 8, 60),  # ('full', 8, 8, 3, False, 4, False)
    ("catalogue", 7, 6, 32, 256, 288, 60),  # ('full', 2, 8, 3, False, 4, True) ('one', False, 1, '49..64')
    ("catalogue", 13, 4, 16, 256, 300, 60),  # ('full', 1, 8, 6, True, 8, True)
    ("catalogue", 13, 4, 25, 256, 36, 60),  # ('full', 2, 8, 6, False, 8, True)
    ("catalogue", 13, 4, 25, 256, 292, 60),  # ('full', 2, 8, 6, True, 8, True)
    ("catalogue", 34, 1, 2, 256, 576, 60),  # ('full', 1, 8, 6, False, 8, False)
    ("catalogue", 34, 1, 3, 256, 300, 60),  # ('full', 1, 8, 6, True, 8, False)
    ("catalogue", 34, 1, 17, 256, 300, 60),  # ('full', 2, 8, 6, True, 8, False)
    ("catalogue", 34, 1, 33, 256, 128, 60),  # ('full', 4, 8, 6, False, 8, False)
    ("catalogue", 34, 1, 48, 256, 292, 60),  # ('full', 4, 8, 6, True, 8, False)
    ("catalogue", 34, 1, 64, 256, 8, 60),  # ('full', 4, 8, 3, False, 8, False)
    ("catalogue", 34, 1, 127, 256, 68, 60),  # ('full', 8, 8, 3, False, 8, False)
    ("catalogue", 27, 2, 2, 256, 1024, 60),  # ('full', 1, 8, 6, False, 8, True) ('one', False, 2, '17..32')
    ("inbatch", 97, 4, 128, 64, 8, 60),  # ('full', 8, 4, 3, False, 4, True) ('one', False, 2, '33..48')
    ("inbatch", 113, 4, 64, 256, 96, 60),  # ('full', 4, 8, 3, False, 8, True) ('one', False, 2, '49..64')
    ("catalogue", 43, 2, 17, 40, 128, 60),  # ('full', 2, 4, 6, False, 8, True)
    ("catalogue", 43, 2, 17, 64, 300, 60),  # ('full', 2, 4, 6, True, 8, True)
    ("catalogue", 43, 2, 48, 64, 36, 60),  # ('full', 4, 4, 6, False, 8, True)
    ("catalogue", 43, 2, 64, 40, 320, 60),  # ('full', 4, 4, 6, True, 8, True)
    ("catalogue", 68, 1, 3, 40, 320, 60),  # ('full', 1, 4, 6, True, 8, False)
    ("catalogue", 68, 1, 16, 40, 36, 60),  # ('full', 1, 4, 6, False, 8, False)
    ("catalogue", 68, 1, 17, 40, 64, 60),  # ('full', 2, 4, 6, False, 8, False)
    ("catalogue", 68, 1, 25, 64, 292, 60),  # ('full', 2, 4, 6, True, 8, False)
    ("catalogue", 68, 1, 48, 40, 36, 60),  # ('full', 4, 4, 6, False, 8, False)
    ("catalogue", 68, 1, 64, 40, 32, 60),  # ('full', 4, 4, 3, False, 8, False)
    ("catalogue", 68, 1, 64, 64, 292, 60),  # ('full', 4, 4, 6, True, 8, False)
    ("catalogue", 68, 1, 100, 40, 4, 60),  # ('full', 8, 4, 3, False, 8, False)
    ("catalogue", 23, 6, 64, 128, 256, 60),  # ('full', 4, 8, 6, False, 8, True) ('several', True, 2, '17..32')
    ("catalogue", 81, 1, 2, 40, 292, 60),  # ('full', 1, 4, 6, True, 8, True) ('several', False, 2, '17..32')
    ("inbatch", 193, 4, 16, 40, 100, 60),  # ('full', 1, 4, 6, False, 8, True) ('several', True, 2, '33..48')
    ("catalogue", 97, 1, 17, 128, 200, 60),  # ('full', 2, 8, 3, False, 8, True) ('several', False, 2, '33..48')
    ("catalogue", 75, 2, 65, 256, 100, 60),  # ('full', 8, 8, 3, False, 8, True) ('several', True, 2, '49..64')
    ("catalogue", 688, 2, 2, 100, 4, 60),  # ('full', 1, 8, 3, False, 8, False) ('capped', False, 3, '<=16')
    ("catalogue", 461, 4, 2, 128, 4, 60),  # ('full', 1, 8, 3, False, 8, True) ('capped', True, 3, '17..32')
    ("catalogue", 580, 3, 2, 40, 4, 60),  # ('full', 1, 4, 3, False, 8, False) ('capped', False, 3, '17..32')
    ("catalogue", 197, 12, 17, 64, 4, 60),  # ('full', 2, 4, 3, False, 8, True) ('capped', True, 3, '33..48')
    ("catalogue", 644, 3, 17, 64, 4, 60),  # ('full', 2, 4, 3, False, 8, False) ('capped', False, 3, '33..48')
    ("catalogue", 939, 2, 33, 40, 4, 60),  # ('full', 4, 4, 3, False, 8, True) ('capped', True, 3, '49..64')
    ("catalogue", 944, 2, 17, 100, 4, 60),  # ('full', 2, 8, 3, False, 8, False) ('capped', False, 3, '49..64')
]

# the widths the invariants are swept over
M_MAX = 8192
T_RANGE = range(2, 129)
WORD_DIMS = range(4, 1025, 4)
TEXT_DIMS = (40, 64, 100, 128, 256)
# every threshold of the launchers +- 1 (T: the position-tile classes; M: the unit count against 4 x 32
# per column-block count, the one-chunk limit, the 16-chunk cap and its neighbours)
T_EDGES = (2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128)
M_EDGES = sorted(set(range(1, 301)) | {383, 384, 385, 511, 512, 513, 1023, 1024, 1025, 1919, 1920, 1921, 2047, 2048,
                                       2049, 2050, 2064, 2065, 2079, 2080, 2081, 4095, 4096, 4097, 8191, 8192})
# word widths: around every LDS limit (288 / 320: TBW 8; 544 / 576: TBW 4), config 4's 300, the
# one- / two-chunk and odd / even chunk counts
WORD_EDGES = (4, 28, 32, 36, 60, 64, 68, 92, 96, 100, 128, 284, 288, 292, 296, 300, 316, 320, 324, 352, 540, 544, 548,
              572, 576, 580, 1020, 1024)


def case_items(c):
    layout, B, N = c[:3]
    return B if layout == "inbatch" else B * (1 + N)


def case_id(c):
    layout, B, N, T, td, wd, V = c
    return "%s-B%d-N%d-T%d-td%d-wd%d" % (layout, B, N, T, td, wd)


def text_dims(nat, T, td, wd, d=32, H=32):
    return nat.make_dims(H, d, 300, 50, TEXT, (td, wd, T, PAD))


class RawShape:
    """dcue_debug_text_shape without the dict (the sweeps call it some 10^5 times): the 16 words."""

    def __init__(self, nat):
        self.nat = nat
        self.f = nat.lib().dcue_debug_text_shape
        self.buf = (ctypes.c_int32 * nat.TEXT_SHAPE_WORDS)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)

    def __call__(self, dims, M):
        st = self.f(ctypes.byref(dims), M, self.p, self.nat.TEXT_SHAPE_WORDS)
        assert st == 0, (st, M)
        return tuple(self.buf)


def _pass_class(n):
    return "<=16" if n <= 16 else "17..32" if n <= 32 else "33..48" if n <= 48 else "49..64"


def fwd_key(w):
    """(kernel, TB / TBW, waves or IPW, BPD, NCH > 0, nxcd, ragged unit tail / short last workgroup)."""
    kernel, tb, wv, nct, bpd, nch, nxcd, units, grid, lds, lds_static, last = w[:12]
    ragged = last < wv if kernel else units % nxcd != 0
    return ("fwd", "chunked" if kernel else "full", tb, wv, bpd, nch > 0, nxcd, ragged)


def wgrad_key(w):
    """(one / several / capped chunks, short last chunk, 64-item staging passes of a full chunk in
    {1, 2, > 2}, items of its last pass by the 16-item load groups)."""
    nchunk, ipc, last, reduce = w[12:16]
    cls = "one" if nchunk == 1 else "capped" if ipc > 128 else "several"
    passes = (ipc + 63) // 64
    return ("wgrad", cls, last < ipc, min(passes, 3), _pass_class(ipc - 64 * (passes - 1)))


def keys_of(w):
    return {fwd_key(w), wgrad_key(w)}


def shape_words(nat, c):
    layout, B, N, T, td, wd, V = c
    return RawShape(nat)(text_dims(nat, T, td, wd), case_items(c))
