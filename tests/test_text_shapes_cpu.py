"""The text branch's launch selection on the host (dcue_debug_text_shape, no GPU): invariants of every
forward kernel / tiling / prefetch depth / XCD spread and every weight-gradient chunking that
M = 1..8,192 items, T = 2..128 positions, word widths 4..1,024 and the text widths can select, and the
closure of tests/test_gpu_text_shapes.py's cases over the variants those shapes select. A threshold of
launch_text_fwd / launch_text_wgrad that moves changes the reachable set: the closure test then fails
until a GPU case covers the new variant."""
import pytest

import text_shape_cases as C

LDS_FULL = 150 * 1024     # k_text_fwd_full's dynamic LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize)
LDS_WG = 160 * 1024       # gfx950 LDS per workgroup
LDS_STATIC = 64 * 1024    # static LDS of a kernel


@pytest.fixture(scope="module")
def nat():
    from dcrecommend import _native
    _native.lib()
    return _native


def _check_fwd(nat, w, M, T, td, wd, where):
    kernel, tb, wv, nct, bpd, nch, nxcd, units, grid, lds, lds_static, last = w[:12]
    EP = (wd + 31) // 32 * 32
    assert tb in (1, 2, 4, 8) and 16 * tb >= T and (tb == 1 or 8 * tb < T), (where, tb)  # the positions: one pass
    if kernel == 0:
        assert lds <= LDS_FULL and lds + lds_static <= LDS_WG, (where, lds)
        assert wv in (4, 8) and nct in (1, 2) and nxcd in (4, 8), where
        nchunk = EP // 32
        assert nch in (0, nchunk) and bpd >= 1 and (3 * nchunk) % bpd == 0, (where, bpd, nchunk)
        assert units % M == 0 and units >= M, where
        Cs = units // M * 16 * wv * nct
        per = -(-units // nxcd)
        assert nxcd * per >= units and grid == 8 * per, (where, units, nxcd, grid)
        # every unit has exactly one block: unit L runs in block (L // per) + 8 (L % per), below the grid
        assert (units - 1) // per < nxcd and (units - 1) % per < grid // 8, where
        assert last == 1, where
    else:
        assert lds == 0 and lds_static <= LDS_STATIC, (where, lds_static)
        assert wv * tb == 8 and nct == 1 and bpd == 0 and nch == 0 and nxcd == 0, where
        rows = -(-M // wv)
        assert units % rows == 0 and grid == units, where
        Cs = units // rows * 64
        assert 1 <= last <= wv and (M - last) % wv == 0 and (M - last) // wv == rows - 1, (where, last)
    assert Cs % 64 == 0 and td <= Cs == nat.text_storage(td), (where, Cs)


@pytest.mark.parametrize("td", C.TEXT_DIMS)
def test_forward_invariants(nat, td):
    """Every word width at the M and T edges, every T at the word-width edges, and the M edges
    (1..300 in full: the unit-count thresholds 64 / 65 and 128 / 129 and every remainder by nxcd and
    IPW) at the T and word-width edges."""
    shape = C.RawShape(nat)
    n = 0
    for T in C.T_RANGE:
        for wd in (C.WORD_DIMS if T in C.T_EDGES else C.WORD_EDGES):
            dims = C.text_dims(nat, T, td, wd)
            wide = T in C.T_EDGES and wd in C.WORD_EDGES
            for M in (C.M_EDGES if wide else (1, 2, 64, 65, 128, 129, 130, C.M_MAX)):
                _check_fwd(nat, shape(dims, M), M, T, td, wd, "M=%d T=%d td=%d wd=%d" % (M, T, td, wd))
                n += 1
    assert n > 100000


def test_wgrad_invariants(nat):
    """The chunks partition [0, M) with none empty, at most 16 of them, and as many as the workspace's
    partials (twpart, the last slice carved: behind tidx [M][C_s] and the part maxima [M][2][C_s] x 8 B,
    256-B aligned) are sized for."""
    shape = C.RawShape(nat)
    for td, wd in ((40, 4), (256, 300)):
        dims = C.text_dims(nat, 16, td, wd)
        Cs = nat.text_storage(td)
        per_chunk = 4 * (Cs * wd * 3 + Cs)
        for M in range(1, C.M_MAX + 1):
            nchunk, ipc, last, reduce = shape(dims, M)[12:16]
            where = "M=%d" % M
            assert 1 <= nchunk <= 16 and reduce == (nchunk > 1), where
            assert (nchunk - 1) * ipc < M <= nchunk * ipc and last == M - (nchunk - 1) * ipc >= 1, (where, nchunk, ipc)
            assert M <= 128 * nchunk or nchunk == 16, where
            if M in C.M_EDGES:
                align = lambda v: (v + 255) // 256 * 256
                tpart = align(nat.workspace_text(dims, 1, 0, M)[2] + M * Cs)
                twpart = align(tpart + 16 * M * Cs)
                room = nat.workspace_bytes(dims, 1, 0, M) - 256 - twpart
                assert room == nchunk * per_chunk, (where, room, nchunk, per_chunk)


def test_report_rejects_bad_arguments(nat):
    import ctypes
    dims = C.text_dims(nat, 16, 40, 8)
    buf = (ctypes.c_int32 * nat.TEXT_SHAPE_WORDS)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = nat.lib().dcue_debug_text_shape
    assert f(ctypes.byref(dims), 5, p, nat.TEXT_SHAPE_WORDS) == 0
    assert f(ctypes.byref(dims), 5, p, nat.TEXT_SHAPE_WORDS - 1) == 1   # cap
    assert f(ctypes.byref(dims), 0, p, nat.TEXT_SHAPE_WORDS) == 1       # M
    assert f(ctypes.byref(dims), 5, None, nat.TEXT_SHAPE_WORDS) == 1
    assert f(None, 5, p, nat.TEXT_SHAPE_WORDS) == 1
    audio = nat.make_dims(32, 32, 300, 50)
    assert f(ctypes.byref(audio), 5, p, nat.TEXT_SHAPE_WORDS) == 1      # no text branch
    off = (ctypes.c_size_t * 3)()
    g = nat.lib().dcue_workspace_text
    assert g(ctypes.byref(dims), 2, 3, 8, off) == 0 and off[0] < off[1] < off[2]
    assert g(ctypes.byref(audio), 2, 3, 8, off) == 1
    assert g(ctypes.byref(dims), 2, 3, 0, off) == 1 and g(ctypes.byref(dims), 2, 3, 8, None) == 1


def test_report_at_config_4(nat):
    """The report names what config 4 is known to run: the bench shape's 64 items on
    eight waves with the ten K chunks at compile time, six weight steps in flight, 128 units on four
    XCDs, one weight-gradient chunk; a 128-position bio at that word width takes the chunked kernel."""
    s = nat.text_shape(C.text_dims(nat, 64, 256, 300, d=256, H=128), 64)
    f, g = s["fwd"], s["wgrad"]
    assert (f["kernel"], f["tb"], f["waves"], f["nct"], f["bpd"], f["nch"], f["nxcd"], f["units"], f["grid"]) == \
        ("full", 4, 8, 1, 6, 10, 4, 128, 256)
    assert f["lds"] == 66 * 712 * 2
    assert g == {"nchunk": 1, "items_per_chunk": 64, "last": 64, "reduce": False}
    s = nat.text_shape(C.text_dims(nat, 128, 256, 300), 130)
    assert (s["fwd"]["kernel"], s["fwd"]["tb"], s["fwd"]["waves"], s["fwd"]["last"]) == ("chunked", 8, 1, 1)
    assert s["wgrad"] == {"nchunk": 2, "items_per_chunk": 65, "last": 65, "reduce": True}


def _reachable(nat):
    """Keys a training step can select: M >= 2 items (a step has a negative per row), at the edges of
    M, T and the word width, every text width; the weight gradient's over every M."""
    shape = C.RawShape(nat)
    reach = {}
    for td in C.TEXT_DIMS:
        for T in C.T_EDGES:
            for wd in C.WORD_EDGES:
                dims = C.text_dims(nat, T, td, wd)
                for M in C.M_EDGES[1:]:
                    reach.setdefault(C.fwd_key(shape(dims, M)), (M, T, td, wd))
    dims = C.text_dims(nat, 16, 40, 4)
    for M in range(2, C.M_MAX + 1):
        reach.setdefault(C.wgrad_key(shape(dims, M)), (M,))
    return reach


def test_gpu_cases_reach_every_variant(nat):
    reach = _reachable(nat)
    covered = set()
    for c in C.CASES:
        covered |= C.keys_of(C.shape_words(nat, c))
    missing = sorted(((k, reach[k]) for k in set(reach) - covered), key=str)
    assert not missing, "%d variants no GPU case runs (key, first (M, T, text_dim, word_dim) reaching it):\n%s" % (
        len(missing), "\n".join(map(str, missing)))


def test_every_case_is_needed(nat):
    """No case is redundant: removing any one leaves a variant uncovered (so the closure test fails
    if a row is taken out of the list)."""
    keys = [C.keys_of(C.shape_words(nat, c)) for c in C.CASES]
    for i, c in enumerate(C.CASES):
        others = set().union(*(k for j, k in enumerate(keys) if j != i))
        assert keys[i] - others, "%s selects no variant the other cases do not" % C.case_id(c)
