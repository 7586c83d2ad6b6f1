"""dcue_crop_tracks_augmented without a GPU: the ABI mirror, every host-side refusal of include/dcue.h,
the host restatement dcue_augment_params_host against tests/augment_reference.py, and the cases the GPU
test's setup has to contain."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import augment_reference as A
import crop_reference as R
from conftest import ROOT


def _nat():
    from dcrecommend import _native as nat
    return nat


# ------------------------------------------------------------------------------------------ ABI
def test_abi_symbols_struct_and_constants(tmp_path):
    nat = _nat()
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert int(re.search(r"#define DCUE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == nat.ABI_VERSION  # the number stays
    for n in ("dcue_crop_tracks_augmented", "dcue_augment_params_host"):
        assert re.search(r"^int %s\(" % n, hdr, flags=re.M), n
        assert n in nat._SIGS and hasattr(nat.lib(), n)
    for macro, val, ref in (("DCUE_AUG_MAX_MASKS", nat.AUG_MAX_MASKS, A.MAX_MASKS),
                            ("DCUE_AUG_FILL_MEAN", nat.AUG_FILL_MEAN, A.FILL_MEAN),
                            ("DCUE_AUG_FILL_CONST", nat.AUG_FILL_CONST, A.FILL_CONST)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, hdr).group(1)) == val == ref
    cname, cls, size = "dcue_augment_config", nat.AugmentConfig, 32
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcue.h"', "int main(void) {",
           'printf("size %%zu\\n", sizeof(%s));' % cname]
    for f, _ in cls._fields_:
        src.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
    src.append("return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == size
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert len(got) == 1 + len(cls._fields_) == 9


def test_augment_config_helper():
    nat = _nat()
    c = nat.augment_config(2, 27, 3, 40, 6.0)
    assert (c.n_freq, c.freq_width, c.n_time, c.time_width, c.gain_db) == (2, 27, 3, 40, 6.0)
    assert (c.fill_mode, c.fill_value, c.reserved) == (nat.AUG_FILL_MEAN, 0.0, 0)
    c = nat.augment_config(fill=-80.0)
    assert (c.fill_mode, c.fill_value) == (nat.AUG_FILL_CONST, -80.0)
    with pytest.raises(ValueError, match="fill"):
        nat.augment_config(fill="median")


# ------------------------------------------------------------------------------------ refusals
def _aug(**kw):
    nat = _nat()
    a = dict(n_freq=2, freq_width=27, n_time=2, time_width=40, gain_db=6.0, fill_mode=0, fill_value=0.0, reserved=0)
    a.update(kw)
    return nat.AugmentConfig(*[a[f] for f, _ in nat.AugmentConfig._fields_])


def _call(aug_kw=None, store_kw=None, cfg_kw=None, n_out=4, out=0x10000000, out_dtype=0, flags=0x20000000, aug=True):
    """dcue_crop_tracks_augmented on made-up addresses: every refusal comes before the call reads a
    pointer or launches, so the status and the text are reached without a GPU."""
    nat = _nat()
    s = dict(data=0x100000, frame_ptr=0x8000000, n_tracks=8, total_frames=1000, dtype=0, reserved=0)
    s.update(store_kw or {})
    c = dict(mode=nat.CROP_RANDOM, seed=0, draw=0, grid_j=0, grid_n=1)
    c.update(cfg_kw or {})
    st = nat.TrackStore(*[s[f] for f, _ in nat.TrackStore._fields_])
    cf = nat.crop_config(**c)
    ag = _aug(**(aug_kw or {}))
    lib = nat.lib()
    launches = lib.dcue_launch_count()
    status = lib.dcue_crop_tracks_augmented(ctypes.byref(st), ctypes.byref(cf), ctypes.byref(ag) if aug else None, None,
                                            n_out, ctypes.c_void_p(out) if out else None, out_dtype, None,
                                            ctypes.c_void_p(flags) if flags else None, None)
    assert lib.dcue_launch_count() == launches
    return status, lib.dcue_last_error().decode()


AUG_REFUSALS = [
    (dict(n_freq=5), "n_freq"), (dict(n_freq=-1), "n_freq"), (dict(n_time=5), "n_time"), (dict(n_time=-1), "n_time"),
    (dict(freq_width=129), "freq_width"), (dict(freq_width=-1), "freq_width"),
    (dict(time_width=132), "time_width"), (dict(time_width=-1), "time_width"),
    (dict(gain_db=-1.0), "gain_db"), (dict(gain_db=float("inf")), "gain_db"), (dict(gain_db=float("nan")), "gain_db"),
    (dict(fill_value=float("inf")), "fill_value"), (dict(fill_mode=1, fill_value=float("nan")), "fill_value"),
    (dict(fill_mode=2), "fill_mode"), (dict(fill_mode=-1), "fill_mode"), (dict(reserved=1), "reserved"),
    # refused even where the rest of the configuration is off
    (dict(n_freq=0, n_time=0, gain_db=0.0, reserved=7), "reserved"),
]


@pytest.mark.parametrize("aug_kw,word", AUG_REFUSALS)
def test_augment_refusals(aug_kw, word):
    status, text = _call(aug_kw=aug_kw)
    assert status == 1 and word in text, (status, text)
    # the host restatement refuses the same configurations
    nat = _nat()
    lengths = np.array([5], dtype=np.int64)
    assert nat.lib().dcue_augment_params_host(ctypes.byref(nat.crop_config(nat.CROP_RANDOM)), ctypes.byref(_aug(**aug_kw)),
                                              ctypes.c_void_p(lengths.ctypes.data), None, 1, None, None, None) == 1
    assert word in nat.lib().dcue_last_error().decode()


@pytest.mark.parametrize("aug", [True, False])
@pytest.mark.parametrize("kw,word", [
    (dict(out=0), "null out"), (dict(flags=0), "null out or flags"), (dict(n_out=-1), "negative"),
    (dict(store_kw=dict(n_tracks=-1)), "negative"), (dict(store_kw=dict(total_frames=-1)), "negative"),
    (dict(cfg_kw=dict(mode=4)), "unknown mode"), (dict(store_kw=dict(dtype=2)), "dtype"), (dict(out_dtype=2), "dtype"),
    (dict(cfg_kw=dict(mode=2, grid_j=3, grid_n=3)), "grid_n"),
    (dict(store_kw=dict(data=0x100008)), "16-byte"), (dict(out=0x10000008), "16-byte"),
    (dict(store_kw=dict(frame_ptr=0)), "frame_ptr"), (dict(store_kw=dict(data=0)), "null store data"),
    (dict(out=0x100000), "overlaps"), (dict(out=0x100000 + 255984), "overlaps"),
])
def test_everything_the_plain_crop_refuses(kw, word, aug):
    status, text = _call(aug=aug, **kw)
    assert status == 1 and word in text, (status, text)


def test_refusal_edges():
    nat = _nat()
    assert _call(n_out=0)[0] == 0 and _call(n_out=0, aug=False)[0] == 0
    status, text = _call(store_kw=dict(total_frames=2 ** 31))
    assert status == 2 and "total_frames" in text
    lib = nat.lib()
    st = nat.TrackStore(0x100000, 0x8000000, 8, 1000, 0, 0)
    ag = _aug()
    assert lib.dcue_crop_tracks_augmented(None, ctypes.byref(nat.crop_config(0)), ctypes.byref(ag), None, 4,
                                          ctypes.c_void_p(0x10000000), 0, None, ctypes.c_void_p(0x20000000), None) == 1
    assert "null store" in lib.dcue_last_error().decode()
    assert lib.dcue_crop_tracks_augmented(ctypes.byref(st), None, ctypes.byref(ag), None, 4, ctypes.c_void_p(0x10000000),
                                          0, None, ctypes.c_void_p(0x20000000), None) == 1
    assert "null config" in lib.dcue_last_error().decode()
    # the limits themselves are accepted
    cfg = nat.crop_config(nat.CROP_RANDOM)
    lengths = np.array([5, -1], dtype=np.int64)
    ok = _aug(n_freq=4, freq_width=128, n_time=4, time_width=131, gain_db=0.0)
    assert lib.dcue_augment_params_host(ctypes.byref(cfg), ctypes.byref(ok), ctypes.c_void_p(lengths.ctypes.data), None, 1,
                                        None, None, None) == 0
    assert lib.dcue_augment_params_host(ctypes.byref(cfg), ctypes.byref(ok), None, None, 0, None, None, None) == 0
    for args, word in (((ctypes.byref(cfg), None, ctypes.c_void_p(lengths.ctypes.data), None, 1), "null augment"),
                       ((None, ctypes.byref(ok), ctypes.c_void_p(lengths.ctypes.data), None, 1), "null config"),
                       ((ctypes.byref(cfg), ctypes.byref(ok), None, None, 1), "null lengths"),
                       ((ctypes.byref(cfg), ctypes.byref(ok), ctypes.c_void_p(lengths.ctypes.data), None, 2), "negative length"),
                       ((ctypes.byref(cfg), ctypes.byref(ok), ctypes.c_void_p(lengths.ctypes.data), None, -1), "negative n")):
        assert lib.dcue_augment_params_host(*args, None, None, None) == 1
        assert word in lib.dcue_last_error().decode(), word


# ----------------------------------------------------------------- the host restatement of the rule
IDS = np.array([0, 1, 7, 36, 199999, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 12345, 2 ** 40], dtype=np.int64)
DRAWS = (0, 1, 2 ** 40, 2 ** 32, 2 ** 32 + 9, 2 ** 64 - 1)


def _check_params(cfg_kw, aug):
    nat = _nat()
    lengths = np.tile(R.LENGTHS, len(IDS))
    ids = np.repeat(IDS, len(R.LENGTHS))
    fill = {} if aug.fill == "mean" else dict(fill=aug.fill)
    got_g, got_f, got_t = nat.augment_params_host(
        nat.crop_config(**cfg_kw), nat.augment_config(aug.n_freq, aug.freq_width, aug.n_time, aug.time_width,
                                                      float(aug.gain_db), **fill), lengths, ids)
    assert got_g.dtype == np.float32 and got_f.shape == got_t.shape == (len(ids), 4, 2)
    for k, (t, L) in enumerate(zip(ids, lengths)):
        g, freq, time = A.params(aug, cfg_kw.get("seed", 0), cfg_kw.get("draw", 0), int(t), int(L))
        assert got_g[k].view(np.int32) == g.view(np.int32), (cfg_kw, k)
        want_f = freq + [(0, 0)] * (4 - len(freq))
        want_t = time + [(0, 0)] * (4 - len(time))
        assert got_f[k].tolist() == [list(x) for x in want_f], (cfg_kw, k)
        assert got_t[k].tolist() == [list(x) for x in want_t], (cfg_kw, k)
        n = min(int(L), R.W)
        assert -aug.gain_db <= g < aug.gain_db or aug.gain_db == 0
        assert all(0 <= w <= aug.freq_width and 0 <= p and p + w <= R.N_MELS for p, w in freq)
        assert all(0 <= w <= min(aug.time_width, n) and 0 <= p and p + w <= n for p, w in time)
    return len(ids)


def test_host_params_equal_the_restatement():
    """72 tracks (9 indices, past 2^31 among them, x every length) x 3 seeds x 6 draws x 5 counts = 6,480
    (seed, draw, t, L), every count from 0 to 4."""
    total = 0
    for seed in (0, 1, 2 ** 63 + 5):
        for draw in DRAWS:
            for count in range(5):
                aug = A.Aug(count, 27, count, 40, 6.0)
                total += _check_params(dict(mode=R.RANDOM, seed=seed, draw=draw), aug)
    assert total == 6480


def test_host_params_widest_masks_other_modes_and_default_ids():
    nat = _nat()
    # the hash is the RANDOM rule's whatever the mode is
    for mode in (R.FIRST, R.CENTER):
        _check_params(dict(mode=mode, seed=3, draw=5), A.Aug(4, 128, 4, 131, 0.5, fill=-80.0))
    _check_params(dict(mode=R.GRID, seed=3, draw=5, grid_j=1, grid_n=3), A.Aug(1, 1, 1, 1, 20.0))
    _check_params(dict(mode=R.RANDOM, seed=3, draw=5), A.Aug(3, 0, 2, 0, 0.0))  # widths 0: every mask empty
    # without ids the index is the position; the time masks stay put when n_freq changes
    cfg = nat.crop_config(nat.CROP_RANDOM, seed=2, draw=3)
    lengths = np.array(R.LENGTHS * 4)
    base = nat.augment_params_host(cfg, nat.augment_config(2, 27, 2, 40, 6.0), lengths)
    same = nat.augment_params_host(cfg, nat.augment_config(2, 27, 2, 40, 6.0), lengths, np.arange(len(lengths)))
    for x, y in zip(base, same):
        assert np.array_equal(x, y)
    other = nat.augment_params_host(cfg, nat.augment_config(4, 27, 2, 40, 6.0), lengths)
    assert np.array_equal(other[2], base[2]) and np.array_equal(other[0], base[0])
    assert np.array_equal(other[1][:, :2], base[1][:, :2]) and other[1][:, 2:].any()
    # another draw, seed or track: another gain
    for kw in (dict(seed=2, draw=4), dict(seed=3, draw=3)):
        g = nat.augment_params_host(nat.crop_config(nat.CROP_RANDOM, **kw), nat.augment_config(gain_db=6.0), lengths)[0]
        assert np.mean(g == base[0]) < 0.1
    assert len(set(base[0].tolist())) == len(lengths)


def test_exact_mean_of_the_restatement():
    """The restatement's own sum: independent of the order, and the case a float sum gets wrong."""
    rs = np.random.RandomState(0)
    x = (rs.randn(131, 128) * 100).astype(np.float16)
    x[0, 0], x[5, 5] = 65504.0, -65504.0
    x[1, 1] = 2.0 ** -24
    m = A.exact_mean(x)
    assert m.view(np.int32) == A.exact_mean(x[::-1, ::-1].copy()).view(np.int32) == A.exact_mean(rs.permutation(x.ravel())).view(np.int32)
    from fractions import Fraction
    want = sum(Fraction(v) for v in x.ravel().tolist()) / x.size
    assert abs(Fraction(float(m)) - want) <= Fraction(float(np.spacing(np.abs(m)))) * Fraction(51, 100)  # two roundings
    assert np.isnan(A.exact_mean(np.array([1.0, np.inf], dtype=np.float16)))
    assert A.exact_mean(np.array([2.0 ** -24, 0.0], dtype=np.float16)) == np.float32(2.0 ** -25)


def test_the_gpu_tests_setup_contains_every_case():
    """The store of tests/test_gpu_augment.py (test_gpu_crop.py's lengths) at its (seed, draw) pairs."""
    rs = np.random.RandomState(4)
    lengths = np.concatenate([R.LENGTHS, rs.choice(R.LENGTHS, 37 - len(R.LENGTHS))])
    lengths = rs.permutation(lengths).astype(np.int64)
    counts, signs = A.case_counts(lengths, A.Aug(gain_db=6.0, **A.CASE_AUG))
    assert counts == A.CASE_COUNTS and {-1, 1} <= signs


# ------------------------------------------------------------------------------- the driver
def test_train_dcue_options():
    import train_dcue
    args = train_dcue.parse(["--synthetic"])
    assert train_dcue.augment_of(args) is None  # off by default
    args = train_dcue.parse(["--synthetic", "--crop", "epoch", "--augment-freq-masks", "2", "--augment-freq-width", "27",
                             "--augment-time-masks", "2", "--augment-time-width", "40", "--augment-gain-db", "6",
                             "--augment-fill", "-80"])
    assert train_dcue.augment_of(args) == dict(freq_masks=2, freq_width=27, time_masks=2, time_width=40, gain_db=6.0,
                                               fill=-80.0)
    args = train_dcue.parse(["--synthetic", "--crop", "epoch", "--augment-gain-db", "3", "--augment-fill", "mean"])
    assert train_dcue.augment_of(args) == dict(gain_db=3.0, fill="mean")
    with pytest.raises(SystemExit):
        train_dcue.parse(["--synthetic", "--augment-fill", "median"])
