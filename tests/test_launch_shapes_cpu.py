"""The launch planners on the host (dcue_debug_launch_shape, no GPU): invariants of every tiling and
split-K partition a training step can select for M = 1..8,192 items, and the closure of
tests/test_gpu_shapes.py's cases over the variants those shapes select -- each (kernel, TW, DEEP, f16,
ragged last tile, tile spanning two items, chunking, CPW, IT, short last workgroup) combination some M
reaches is run against the fp64 oracle by at least one GPU case. A planner threshold that moves
changes the reachable set: this test then fails until a case covers the new variant."""
import pytest

import launch_shape_cases as C

LDS_BYTES = 160 * 1024            # gfx950 LDS per workgroup
CHAN_LDS = (5 * 256 + 4) * 4      # conv_rows.h ChanLds, static LDS beside the slab
# (ks, pad, pool, Lin, Lp) per conv layer (dcue_common.h layer_geom; oracle CONV_SPECS)
GEOM = {1: (4, 2, 4, 131, 33), 2: (4, 2, 4, 33, 8), 3: (4, 2, 4, 8, 2), 4: (2, 1, 2, 2, 1), 5: (1, 0, 1, 1, 1)}
F16_KERNELS = ("wgrad16t", "multi_f16")
K_WG_ITEMS = 128                  # conv_wgrad.hip kWgItems: the tap-fused conv-1 kernel's LDS item table


def _storage(w):
    return 32 if w <= 32 else 64 if w <= 64 else 128 if w <= 128 else 256


def _slab_fits(R, ks, kc, tw):
    rows = 16 * tw
    return (rows + ((rows + R - 1) // R + 1) * (ks - 1)) * (kc + 8) * 4 + CHAN_LDS <= LDS_BYTES


@pytest.fixture(scope="module")
def nat():
    from dcrecommend import _native
    _native.lib()
    return _native


@pytest.mark.parametrize("H,d", C.WIDTHS)
def test_planner_invariants(nat, H, d):
    dims = nat.make_dims(H, d, 300, 50)
    Hs, Ds = _storage(H), _storage(d)
    for M in range(1, C.M_MAX + 1):
        for layout, B, N in ((C.CATALOGUE, M, 0), (C.GATHER, 1, 1)):  # the planners see only M
            s = nat.launch_shape(dims, layout, B, N, M)
            where = "M=%d layout=%d H=%d d=%d" % (M, layout, H, d)
            for kind in ("fwd", "dgrad"):
                for l, (tw, deep, f16, last, spans) in s[kind].items():
                    ks, pad, pool, lin, lp = GEOM[l]
                    R = lp * pool if kind == "fwd" else lin
                    kc = 128 if (kind, l) == ("fwd", 1) else Ds if (kind, l) == ("dgrad", 5) else Hs
                    assert tw in (1, 2, 3, 4, 8) and _slab_fits(R, ks, kc, tw), (where, kind, l, tw)
                    assert last == (M * R) % (16 * tw) and (not deep or tw == 1), (where, kind, l)
            for l, (kernel, nchunk, rpc, last) in s["wgrad"].items():
                ks, pad, pool, lin, lp = GEOM[min(l, 5)]
                rows = M * lp * pool
                assert nchunk >= 1, (where, l)
                assert (nchunk - 1) * rpc < rows <= nchunk * rpc, (where, l, nchunk, rpc, rows)
                assert last == rows - (nchunk - 1) * rpc, (where, l)
                if kernel in F16_KERNELS:
                    assert rpc % 64 == 0, (where, l, rpc)
                if kernel == "conv1_wgrad":
                    assert rpc % pool == 0, (where, l, rpc)
                if l == 1 and kernel == "wgrad16t":
                    assert rpc // 132 + 3 <= K_WG_ITEMS, (where, rpc)
            cpw, kernel, it, wlds, last = s["tail"]
            assert cpw in (0, 4, 8) and it in (1, 2, 4, 16) and 1 <= last <= it and (M - last) % it == 0, where


@pytest.mark.parametrize("H,d", C.WIDTHS)
def test_workspace_grows_with_items(nat, H, d):
    dims = nat.make_dims(H, d, 300, 50)
    for B, N in ((1, 0), (1024, 40)):
        best = 0
        for M in range(1, C.M_MAX + 1):
            n = nat.workspace_bytes(dims, B, N, M)
            assert n >= best, "workspace for M=%d (%d B) below a smaller M's (%d B) at H=%d d=%d" % (M, n, best, H, d)
            best = n


def test_report_rejects_bad_arguments(nat):
    import ctypes
    dims = nat.make_dims(32, 32, 300, 50)
    buf = (ctypes.c_int32 * nat.LAUNCH_SHAPE_WORDS)()
    f = nat.lib().dcue_debug_launch_shape
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert f(ctypes.byref(dims), C.CATALOGUE, 2, 3, 8, p, nat.LAUNCH_SHAPE_WORDS) == 0
    assert f(ctypes.byref(dims), C.CATALOGUE, 2, 3, 8, p, nat.LAUNCH_SHAPE_WORDS - 1) == 1   # cap
    assert f(ctypes.byref(dims), C.CATALOGUE, 2, 3, 7, p, nat.LAUNCH_SHAPE_WORDS) == 1       # M != B(1+N)
    assert f(ctypes.byref(dims), C.GATHER, 4, 3, 3, p, nat.LAUNCH_SHAPE_WORDS) == 1          # M < B
    assert f(ctypes.byref(dims), 7, 2, 3, 8, p, nat.LAUNCH_SHAPE_WORDS) == 1                 # layout
    assert f(ctypes.byref(dims), C.CATALOGUE, 2, 3, 8, None, nat.LAUNCH_SHAPE_WORDS) == 1
    assert f(None, C.CATALOGUE, 2, 3, 8, p, nat.LAUNCH_SHAPE_WORDS) == 1


def test_report_at_the_bench_shape(nat):
    """The report names what the bench shape is known to run: in-batch M = 64
    one-tile DEEP forwards past conv 1, the tap-fused conv-1 / conv-2 weight gradients; catalogue
    M = 1,344 eight tiles per workgroup on conv 1 and a split-f16 layer-2 input gradient."""
    dims = nat.make_dims(128, 128, 300, 400)
    s = nat.launch_shape(dims, C.GATHER, 64, 20, 64)
    assert s["fwd"][1][0] == 3 and s["fwd"][2][:2] == (1, 1)
    assert s["wgrad"][1][0] == "wgrad16t" and s["wgrad"][2][0] == "wgrad16t" and s["wgrad"][6][0] == "multi_f16"
    assert s["dgrad"][2][2] == 0 and s["tail"][:3] == (8, 0, 1)
    s = nat.launch_shape(dims, C.CATALOGUE, 64, 20, 1344)
    assert s["fwd"][1][0] == 8 and s["dgrad"][2][2] == 1 and s["tail"][:3] == (8, 0, 16)


def test_gpu_cases_reach_every_variant(nat):
    """Reachable: by a training step on M = 2..8,192 items (launch_shape_cases.step_batches: M = 1 is
    no step -- no negatives, and BatchNorm over one value per channel) at each (H, d, tower) the GPU
    cases use; the score kernel's CPW by N = 1..1,024."""
    widths = sorted({(c[5], c[4], c[1]) for c in C.CASES})
    reachable = {}
    for H, d, mt in widths:
        dims = nat.make_dims(H, d, 300, 50, mt)
        for M in range(2, C.M_MAX + 1):
            for layout, B, N in C.step_batches(M):
                for k in C.conv_keys(nat.launch_shape(dims, layout, B, N, M)):
                    reachable.setdefault(k, (H, d, mt, layout, M))
    dims = nat.make_dims(32, 32, 300, 50)
    for N in range(1, C.N_MAX + 1):
        reachable.setdefault(C.score_key(nat.launch_shape(dims, C.CATALOGUE, 1, N, 1 + N)), (32, 32, C.BN, 0, 1 + N))
    covered = set()
    for c in C.CASES:
        covered |= C.keys_of(C.shape_of(nat, c))
    missing = sorted((k, reachable[k]) for k in set(reachable) - covered)
    assert not missing, "%d variants no GPU case runs (key, first (H, d, tower, layout, M) reaching it):\n%s" % (
        len(missing), "\n".join(map(str, missing)))
