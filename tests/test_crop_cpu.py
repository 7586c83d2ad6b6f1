"""dcue_crop_tracks without a GPU: the ABI mirror, every host-side refusal of include/dcue.h, the host
restatement dcue_crop_starts_host against tests/crop_reference.py, the RANDOM rule's range and
uniformity, and the kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import crop_reference as R
from conftest import ROOT
from kernel_resources import kernel_resources

LENGTHS = R.LENGTHS + (2 ** 31 // 128,)
DRAWS = (0, 1, 2 ** 40)


def _nat():
    from dcrecommend import _native as nat
    return nat


# ------------------------------------------------------------------------------------------ ABI
def test_abi_symbols_structs_and_constants(tmp_path):
    nat = _nat()
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == nat.ABI_VERSION
    assert nat.lib().dcue_abi_version() == 17
    for n in ("dcue_crop_tracks", "dcue_crop_starts_host"):
        assert re.search(r"^int %s\(" % n, hdr, flags=re.M), n
        assert n in nat._SIGS and hasattr(nat.lib(), n)
    for macro, val, ref in (("DCUE_CROP_FIRST", nat.CROP_FIRST, R.FIRST), ("DCUE_CROP_CENTER", nat.CROP_CENTER, R.CENTER),
                            ("DCUE_CROP_GRID", nat.CROP_GRID, R.GRID), ("DCUE_CROP_RANDOM", nat.CROP_RANDOM, R.RANDOM),
                            ("DCUE_CROP_FLAG_BAD_EXTENT", nat.CROP_FLAG_BAD_EXTENT, R.FLAG_BAD_EXTENT),
                            ("DCUE_CROP_FLAG_BAD_ROW", nat.CROP_FLAG_BAD_ROW, R.FLAG_BAD_ROW)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, hdr).group(1)) == val == ref
    assert nat.CROP_FACTOR_DRAW0 == R.FACTOR_DRAW0 == 2 ** 32
    assert nat.N_FRAMES == R.W and nat.N_MELS == R.N_MELS
    structs = (("dcue_track_store", nat.TrackStore, 40), ("dcue_crop_config", nat.CropConfig, 32))
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcue.h"', "int main(void) {"]
    for cname, cls, _ in structs:
        src.append('printf("%s.size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    src.append("return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    for cname, cls, size in structs:
        assert int(got[cname + ".size"]) == ctypes.sizeof(cls) == size
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)


# ------------------------------------------------------------------------------------ refusals
def _call(store_kw=None, cfg_kw=None, n_out=4, out=0x10000000, out_dtype=0, flags=0x20000000, store=True, cfg=True):
    """dcue_crop_tracks on made-up addresses: every refusal comes before the call reads a pointer or
    launches, so the status and the text are reached without a GPU."""
    nat = _nat()
    s = dict(data=0x100000, frame_ptr=0x8000000, n_tracks=8, total_frames=1000, dtype=0, reserved=0)
    s.update(store_kw or {})
    c = dict(mode=nat.CROP_RANDOM, seed=0, draw=0, grid_j=0, grid_n=1)
    c.update(cfg_kw or {})
    st = nat.TrackStore(*[s[f] for f, _ in nat.TrackStore._fields_])
    cf = nat.crop_config(**c)
    lib = nat.lib()
    launches = lib.dcue_launch_count()
    status = lib.dcue_crop_tracks(ctypes.byref(st) if store else None, ctypes.byref(cf) if cfg else None, None, n_out,
                                  ctypes.c_void_p(out) if out else None, out_dtype, None,
                                  ctypes.c_void_p(flags) if flags else None, None)
    assert lib.dcue_launch_count() == launches
    return status, lib.dcue_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(store=False), "null store"), (dict(cfg=False), "null config"), (dict(out=0), "null out"),
    (dict(flags=0), "null out or flags"),
    (dict(n_out=-1), "negative"), (dict(store_kw=dict(n_tracks=-1)), "negative"),
    (dict(store_kw=dict(total_frames=-1)), "negative"),
    (dict(cfg_kw=dict(mode=4)), "unknown mode"), (dict(cfg_kw=dict(mode=-1)), "unknown mode"),
    (dict(store_kw=dict(dtype=2)), "dtype"), (dict(out_dtype=2), "dtype"), (dict(out_dtype=-1), "dtype"),
    (dict(cfg_kw=dict(mode=2, grid_j=3, grid_n=3)), "grid_n"), (dict(cfg_kw=dict(mode=2, grid_j=0, grid_n=0)), "grid_n"),
    (dict(cfg_kw=dict(mode=2, grid_j=-1, grid_n=3)), "grid_n"),
    (dict(store_kw=dict(data=0x100008)), "16-byte"), (dict(out=0x10000008), "16-byte"),
    (dict(store_kw=dict(frame_ptr=0)), "frame_ptr"), (dict(store_kw=dict(data=0)), "null store data"),
    # out [4][131][128] fp16 = 134,144 bytes; the store's data [1000][128] fp16 = 256,000 bytes from 0x100000
    (dict(out=0x100000), "overlaps"), (dict(out=0x100000 + 255984), "overlaps"),
    (dict(out=0x100000 - 134144 + 16), "overlaps"),
])
def test_refusals(kw, word):
    status, text = _call(**kw)
    assert status == 1 and word in text, (status, text)


def test_refusal_edges():
    nat = _nat()
    # n_out == 0 is DCUE_OK, and so is nothing to do in the host restatement
    assert _call(n_out=0)[0] == 0
    assert nat.lib().dcue_crop_starts_host(ctypes.byref(nat.crop_config(nat.CROP_FIRST)), None, None, 0, None) == 0
    # starts are int32: a store beyond 2^31 - 1 frames is unsupported, not invalid
    status, text = _call(store_kw=dict(total_frames=2 ** 31))
    assert status == 2 and "total_frames" in text
    lengths = np.array([5, -1], dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    cfg = nat.crop_config(nat.CROP_CENTER)
    assert nat.lib().dcue_crop_starts_host(ctypes.byref(cfg), ctypes.c_void_p(lengths.ctypes.data), None, 2,
                                           ctypes.c_void_p(out.ctypes.data)) == 1
    assert "negative length" in nat.lib().dcue_last_error().decode()
    assert nat.lib().dcue_crop_starts_host(ctypes.byref(cfg), None, None, 2, ctypes.c_void_p(out.ctypes.data)) == 1
    assert nat.lib().dcue_crop_starts_host(None, None, None, 0, None) == 1
    bad = nat.crop_config(nat.CROP_GRID, grid_j=2, grid_n=2)
    assert nat.lib().dcue_crop_starts_host(ctypes.byref(bad), ctypes.c_void_p(lengths.ctypes.data), None, 1,
                                           ctypes.c_void_p(out.ctypes.data)) == 1


# ----------------------------------------------------------------- the host restatement of the rule
def _ids(n):
    return np.array([0, 1, 7, 36, 199999, 2 ** 31 - 1, 2 ** 40, 3, 5][:n], dtype=np.int64)


@pytest.mark.parametrize("mode,kws", [
    (R.FIRST, [dict()]), (R.CENTER, [dict()]),
    (R.GRID, [dict(grid_j=j, grid_n=n) for n in (1, 2, 3, 10) for j in range(n)]),
    (R.RANDOM, [dict(seed=s, draw=d) for s in (0, 1, 2 ** 63 + 5) for d in DRAWS + (2 ** 32, 2 ** 32 + 9, 2 ** 64 - 1)]),
])
def test_host_starts_equal_the_restatement(mode, kws):
    nat = _nat()
    for kw in kws:
        cfg = nat.crop_config(mode, **kw)
        for ids in (None, _ids(len(LENGTHS))):
            got = nat.crop_starts_host(cfg, LENGTHS, ids)
            want = R.starts(mode, LENGTHS, ids, **kw)
            assert np.array_equal(got, want), (mode, kw, got, want)
            span = np.maximum(np.array(LENGTHS) - R.W, 0)
            assert np.all((0 <= got) & (got <= span))
            always_first = R.W + 1 if mode == R.RANDOM else R.W  # RANDOM never draws the last window
            assert not got[np.array(LENGTHS) <= always_first].any()


def test_grid_ends_and_center():
    nat = _nat()
    n = 10
    first = nat.crop_starts_host(nat.crop_config(nat.CROP_GRID, grid_j=0, grid_n=n), LENGTHS)
    last = nat.crop_starts_host(nat.crop_config(nat.CROP_GRID, grid_j=n - 1, grid_n=n), LENGTHS)
    assert not first.any()
    assert np.array_equal(last, np.maximum(np.array(LENGTHS) - R.W, 0))  # the last window, exactly
    one = nat.crop_starts_host(nat.crop_config(nat.CROP_GRID, grid_j=0, grid_n=1), LENGTHS)
    assert np.array_equal(one, nat.crop_starts_host(nat.crop_config(nat.CROP_CENTER), LENGTHS))
    steps = [nat.crop_starts_host(nat.crop_config(nat.CROP_GRID, grid_j=j, grid_n=n), [1292])[0] for j in range(n)]
    assert steps == sorted(steps) and len(set(steps)) == n


def test_vectorised_restatement_is_the_scalar_one():
    ts = np.array([0, 1, 5, 2 ** 31 - 1, 2 ** 40], dtype=np.int64)
    for span in (1, 7, 1161, 2 ** 31 // 128 - R.W):
        for seed in (0, 3, 2 ** 64 - 1):
            for draw in DRAWS:
                want = [R.start(R.RANDOM, span + R.W, int(t), seed=seed, draw=draw) for t in ts]
                assert R.random_starts_np(span, seed, np.full(len(ts), draw, dtype=np.uint64), ts).tolist() == want


def _pairs():
    """70,000 (draw, t) pairs: 350 draws (epochs, then the factor passes' draws) x 200 tracks."""
    draws = np.concatenate([np.arange(340), R.FACTOR_DRAW0 + np.arange(10)]).astype(np.uint64)
    ts = np.arange(200, dtype=np.int64) * 997
    return np.repeat(draws, len(ts)), np.tile(ts, len(draws))


def test_random_never_draws_the_last_window_and_is_uniform():
    """L - W = 7 over 70,000 (draw, t) pairs: start 7 -- the reference's exclusive high end -- never
    comes, and every bin of 0..6 lies within 5 standard deviations of 10,000 (sigma = sqrt(70000 * 1/7 * 6/7)
    = 92.6). The restatement is held to the bound first, then the library to the restatement."""
    nat = _nat()
    draws, ts = _pairs()
    assert len(draws) == 70000
    sigma = np.sqrt(70000.0 * (1.0 / 7.0) * (6.0 / 7.0))
    for seed in (0, 12345):
        want = R.random_starts_np(7, seed, draws, ts)
        counts = np.bincount(want, minlength=8)
        print("seed %d bin counts %s (5 sigma = %.0f)" % (seed, counts.tolist(), 5 * sigma))
        assert counts[7] == 0 and counts.sum() == 70000
        assert np.all(np.abs(counts[:7] - 10000.0) <= 5 * sigma), counts
        got = np.empty(70000, dtype=np.int64)
        for d in np.unique(draws):
            sel = draws == d
            got[sel] = nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=seed, draw=int(d)),
                                            np.full(int(sel.sum()), R.W + 7), ts[sel])
        assert np.array_equal(got, want)
    # L = W + 1: always 0
    assert not nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=9, draw=4), np.full(1000, R.W + 1)).any()


def test_draw_seed_and_track_each_change_the_sequence():
    nat = _nat()
    L = np.full(64, 1292)
    ts = np.arange(64)
    base = nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=5), L, ts)
    assert np.array_equal(base, nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=5), L, ts))
    for other in (nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=6), L, ts),
                  nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=4, draw=5), L, ts),
                  nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=5), L, ts + 64),
                  # (seed, draw) are not interchangeable, and neither are (draw, t)
                  nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=5, draw=3), L, ts)):
        assert np.mean(other == base) < 0.1
    swapped = [nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=int(t)), [1292], [5])[0] for t in ts]
    assert np.mean(np.array(swapped) == base) < 0.1
    # the start belongs to the track, not to the position it is asked at
    perm = np.random.RandomState(0).permutation(64)
    assert np.array_equal(nat.crop_starts_host(nat.crop_config(nat.CROP_RANDOM, seed=3, draw=5), L, ts[perm]), base[perm])


# --------------------------------------------------------------------------- kernel resources
def test_crop_kernels_use_no_scratch_and_no_lds(tmp_path):
    res = {k: v for k, v in kernel_resources("crop.hip", tmp_path).items() if "k_crop_tracks" in k}
    assert len(res) == 4, sorted(res)  # one instance per (store dtype, out dtype)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)


# ------------------------------------------------------------------------------- the driver
def test_train_dcue_options():
    import train_dcue
    args = train_dcue.parse(["--synthetic"])
    assert (args.crop, args.crop_seed, args.factor_crops) == ("load", 0, "random")  # today's path by default
    args = train_dcue.parse(["--synthetic", "--crop", "epoch", "--crop-seed", "7", "--factor-crops", "grid"])
    assert (args.crop, args.crop_seed, args.factor_crops) == ("epoch", 7, "grid")
    with pytest.raises(SystemExit):
        train_dcue.parse(["--synthetic", "--crop", "batch"])
