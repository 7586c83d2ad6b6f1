"""dcue_crop_tracks_augmented on the GPU against tests/augment_reference.py, bit for bit (NaNs as NaNs):
the rule fixes every rounding and the mean's sum is exact, so there is no tolerance.

The store is tests/test_gpu_crop.py's: 37 tracks whose lengths are drawn from crop_reference.LENGTHS with
RandomState(4). Every configuration runs at that file's three launch shapes -- 37 rows (16 parts per
row), 300 rows with repeats (4 parts), 2,100 rows (whole rows, kept in registers while the workgroup
sums them, and the strided loop) -- into guarded sentinel rows."""
import ctypes

import numpy as np
import pytest
import torch

import augment_reference as A
import crop_reference as R
import test_gpu_crop as C

pytestmark = pytest.mark.gpu
DEV = C.DEV
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (store dtype, out dtype)
SHAPES = (None, 300, 2100)  # rows: None is the 37 tracks in order
CONFIGS = {"freq": dict(n_freq=2, freq_width=27), "time": dict(n_time=2, time_width=40), "gain": dict(gain_db=6.0),
           "all": dict(gain_db=6.0, **A.CASE_AUG), "four": dict(n_freq=4, freq_width=20, n_time=4, time_width=30, gain_db=1.5)}
FILLS = ("mean", 0.0, -80.0)
KW = dict(seed=7, draw=2 ** 40)
INT = {torch.float16: torch.int16, torch.float32: torch.int32}
_WANT = {}


def _nat_cfg(aug):
    from dcrecommend import _native as nat
    return nat.augment_config(aug.n_freq, aug.freq_width, aug.n_time, aug.time_width, float(aug.gain_db), fill=aug.fill)


def _rows(n):
    return None if n is None else C._rows(n, seed=n)


def _run(dt, odt, aug, mode, kw, rows, data=None, frame_ptr=None, plain=False):
    """One guarded call: (out, starts, flags) on the device. aug: an A.Aug, None (a null pointer), or with
    plain=True dcue_crop_tracks itself."""
    from dcrecommend import _native as nat
    _, _, d, fp = C._store(dt)
    d = d if data is None else data
    fp = fp if frame_ptr is None else frame_ptr
    n = C.N_TRACKS if rows is None else len(rows)
    g = C._Guarded(n, odt)
    out, starts, flags = g.views()
    r = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(DEV)
    cfg = nat.crop_config(mode, **kw)
    if plain:
        nat.crop_tracks(d, fp, cfg, out, rows=r, starts=starts, flags=flags)
    else:
        store = nat.track_store(d, fp)
        ag = None if aug is None else _nat_cfg(aug)
        nat.check(nat.lib().dcue_crop_tracks_augmented(ctypes.byref(store), ctypes.byref(cfg),
                                                       None if ag is None else ctypes.byref(ag), nat.ptr(r), n, nat.ptr(out),
                                                       odt, nat.ptr(starts), nat.ptr(flags), nat.stream_handle()),
                  "dcue_crop_tracks_augmented")
    torch.cuda.synchronize()
    g.check()
    return out, starts, flags


def _want(dt, odt, aug, mode=R.RANDOM, kw=KW):
    """The restatement's table of the 37 tracks, made once per case: (numpy triple, out on the device)."""
    key = (dt, odt, aug.key(), mode, tuple(sorted(kw.items())))
    if key not in _WANT:
        data, fp = C._store(dt)[:2]
        w = A.crop(data, fp, None, C.NP_DTYPE[odt], aug, mode=mode, **kw)
        _WANT[key] = (w, torch.from_numpy(w[0]).to(DEV))
    return _WANT[key]


def _equal_bits(a, b):
    return torch.equal(a.contiguous().view(INT[a.dtype]), b.contiguous().view(INT[b.dtype]))


def _check_all_shapes(dt, odt, aug, mode=R.RANDOM, kw=KW):
    (_, want_starts, _), want = _want(dt, odt, aug, mode, kw)
    lengths = C._lengths()
    for n in SHAPES:
        rows = _rows(n)
        sel = np.arange(C.N_TRACKS) if rows is None else rows
        out, starts, flags = _run(dt, odt, aug, mode, kw, rows)
        assert not flags.any(), (n, aug.key())
        assert np.array_equal(starts.cpu().numpy(), want_starts[sel]), (n, aug.key())
        assert _equal_bits(out, want[torch.from_numpy(sel.astype(np.int64)).to(DEV)]), (n, aug.key())
        if n is None:  # the zero tail of a short track is never touched: bit pattern 0
            for t in np.flatnonzero(lengths < R.W):
                assert not out[t, lengths[t]:].view(INT[out.dtype]).any()


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("dt,odt", PAIRS)
def test_rule_bit_for_bit(dt, odt, name):
    for fill in FILLS:
        _check_all_shapes(dt, odt, A.Aug(fill=fill, **CONFIGS[name]))
    if dt == 1 and name == "all":
        # the fp32 store holds values fp16 cannot: the mean of the elements as stored is another number
        # than the mean of the elements rounded to fp16 first, so that clause of the rule is exercised
        data, fp = C._store(1)[:2]
        differ = 0
        for t in np.flatnonzero(C._lengths() > 0):
            s = R.start(R.RANDOM, fp[t + 1] - fp[t], t, **KW)
            src = data[fp[t] + s:fp[t] + s + min(fp[t + 1] - fp[t], R.W)]
            differ += np.float32(src.astype(np.float64).mean()) != A.exact_mean(src.astype(np.float16))
        assert differ > 0
    if name == "all":  # the augmentation does something: masked and shifted elements, and untouched tails
        plain = R.crop(*C._store(dt)[:2], None, C.NP_DTYPE[odt], R.RANDOM, **KW)[0]
        got = _want(dt, odt, A.Aug(fill=-80.0, **CONFIGS[name]))[0][0]
        assert (got == -80.0).sum() > 1000 and np.mean(got != plain) > 0.3


@pytest.mark.parametrize("dt,odt", PAIRS)
def test_cases_that_must_occur(dt, odt):
    """2 frequency masks <= 27, 2 time masks <= 40 at four (seed, draw): by the restatement the store then
    holds every edge of the rule, the counts asserted first so that a change of rule or seeds cannot
    silently empty the test."""
    aug = A.Aug(gain_db=6.0, **A.CASE_AUG)
    counts, signs = A.case_counts(C._lengths(), aug)
    assert counts == A.CASE_COUNTS and {-1, 1} <= signs
    for seed, draw in A.CASE_PAIRS:
        _check_all_shapes(dt, odt, aug, kw=dict(seed=seed, draw=draw))


@pytest.mark.parametrize("dt,odt", [(0, 0), (1, 0), (1, 1)])
def test_a_track_gives_the_same_row_in_any_position_and_launch_shape(dt, odt):
    """The exact sum: a float reduction would give the 16-part, the 4-part and the whole-row launches
    different means."""
    aug = A.Aug(gain_db=6.0, **A.CASE_AUG)
    base, base_starts, _ = _run(dt, odt, aug, R.RANDOM, KW, None)
    for n in SHAPES[1:]:
        rows = _rows(n)
        out, starts, _ = _run(dt, odt, aug, R.RANDOM, KW, rows)
        idx = torch.from_numpy(rows.astype(np.int64)).to(DEV)
        assert _equal_bits(out, base[idx]) and torch.equal(starts, base_starts[idx])
        assert len(set(rows.tolist())) == C.N_TRACKS and len(rows) > C.N_TRACKS  # every track, and repeats
    # another mode keeps the masks and the gain (the hash is the RANDOM rule's whatever the mode) and moves the window
    first, _, _ = _run(dt, odt, A.Aug(fill=-80.0, **A.CASE_AUG), R.FIRST, KW, None)
    rand, _, _ = _run(dt, odt, A.Aug(fill=-80.0, **A.CASE_AUG), R.RANDOM, KW, None)
    assert torch.equal(first == -80.0, rand == -80.0) and not _equal_bits(first, rand)
    _check_all_shapes(dt, odt, aug, mode=R.CENTER)


@pytest.mark.parametrize("dt,odt", PAIRS)
def test_off_is_todays_path(dt, odt):
    lengths = C._lengths()
    for mode, kw in C.MODES:
        for n in SHAPES:
            rows = _rows(n)
            want = _run(dt, odt, None, mode, kw, rows, plain=True)
            for aug in (None, A.Aug(), A.Aug(n_freq=3, n_time=2), A.Aug(freq_width=27, time_width=40, fill=-80.0)):
                got = _run(dt, odt, aug, mode, kw, rows)
                assert _equal_bits(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
            if n is None:
                for t in np.flatnonzero(lengths < R.W):
                    assert not got[0][t, lengths[t]:].view(INT[got[0].dtype]).any()


def _same(a, b):
    """Bit for bit, NaNs as NaNs."""
    return np.array_equal(C._bits(a), C._bits(b)) or bool(np.all((C._bits(a) == C._bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("dt,odt", [(0, 0), (1, 1), (0, 1)])
def test_one_infinity_makes_the_mean_fill_nan_and_nothing_else(dt, odt):
    aug = A.Aug(gain_db=6.0, **A.CASE_AUG)
    host, fp, dev, _ = C._store(dt)
    lengths = C._lengths()
    t = int(np.flatnonzero(lengths == 1292)[0])
    s = R.start(R.RANDOM, 1292, t, **KW)
    g, freq, time = A.params(aug, KW["seed"], KW["draw"], t, 1292)
    m = A.mask(aug, freq, time, R.W)
    frame, mel = [int(v[0]) for v in np.nonzero(~m)]  # an unmasked element: the inf itself stays inf + g
    assert m.any() and not m.all() and 0 < s < 1292 - R.W - 1
    clean = A.crop(host, fp, None, C.NP_DTYPE[odt], aug, **KW)[0]
    for where, inside in ((fp[t] + s + frame, True), (fp[t] + s - 1, False), (fp[t] + s + R.W, False)):
        data = host.copy()
        data[where, mel] = np.inf
        want = A.crop(data, fp, None, C.NP_DTYPE[odt], aug, **KW)[0]
        for n in SHAPES:
            rows = _rows(n)
            sel = np.arange(C.N_TRACKS) if rows is None else rows
            out = _run(dt, odt, aug, R.RANDOM, KW, rows, data=torch.from_numpy(data).to(DEV))[0].cpu().numpy()
            assert _same(out, want[sel])
            hit = sel == t
            assert np.array_equal(C._bits(out[~hit]), C._bits(clean[sel][~hit]))  # no other row changes by a bit
            if not inside:
                assert np.array_equal(C._bits(out), C._bits(clean[sel]))
                continue
            row = out[hit][0]
            assert np.isnan(row[m]).all() and np.isposinf(row[frame, mel])
            rest = ~m
            rest[frame, mel] = False
            x = data[fp[t] + s:fp[t] + s + R.W].astype(np.float32)
            assert np.array_equal(C._bits(row[rest]), C._bits((x[rest] + g).astype(C.NP_DTYPE[odt])))
            assert np.isfinite(row[rest]).all()


@pytest.mark.parametrize("dt,odt", [(0, 0), (1, 1), (0, 1)])
def test_corrupt_extents_and_rows_are_flagged_and_zero(dt, odt):
    """tests/test_gpu_crop.py's corruptions under the augmenting kernel: the flagged rows come back zero
    with their flags, every other row unchanged, nothing outside `out` written."""
    aug = A.Aug(gain_db=6.0, **A.CASE_AUG)
    data, fp_host, _, _ = C._store(dt)
    for n_rows in (50, 1100):  # 8 parts per row; whole rows
        rows = C._rows(n_rows, seed=8)
        clean = [x.cpu().numpy() for x in _run(dt, odt, aug, R.RANDOM, KW, rows)]
        for entry, value, bad_tracks in ((C.N_TRACKS, len(data) + 5, {C.N_TRACKS - 1}), (11, -3, {10, 11})):
            for bad_row_value in (C.N_TRACKS, -1, 2 ** 31 - 1):
                fp = fp_host.copy()
                fp[entry] = value
                r = rows.copy()
                victim = int(np.flatnonzero(~np.isin(rows, list(bad_tracks)))[5])
                r[victim] = bad_row_value
                want, want_starts, want_flags = A.crop(data, fp, r, C.NP_DTYPE[odt], aug, total_frames=len(data), **KW)
                out, starts, flags = [x.cpu().numpy() for x in
                                      _run(dt, odt, aug, R.RANDOM, KW, r, frame_ptr=torch.from_numpy(fp).to(DEV))]
                assert np.array_equal(flags, want_flags)
                hit = np.isin(rows, list(bad_tracks))
                assert hit.any() and np.all(flags[hit] == R.FLAG_BAD_EXTENT) and flags[victim] == R.FLAG_BAD_ROW
                flagged = hit.copy()
                flagged[victim] = True
                assert not flags[~flagged].any()
                assert not C._bits(out[flagged]).any() and not starts[flagged].any()
                assert np.array_equal(C._bits(out[~flagged]), C._bits(clean[0][~flagged]))
                assert np.array_equal(starts[~flagged], clean[1][~flagged])
                assert np.array_equal(C._bits(out), C._bits(want)) and np.array_equal(starts, want_starts)
    # without rows, an output row past the last track is a bad row
    from dcrecommend import _native as nat
    _, _, ddata, dfp = C._store(dt)
    g = C._Guarded(C.N_TRACKS + 3, odt)
    out, starts, flags = g.views()
    nat.crop_tracks(ddata, dfp, nat.crop_config(R.RANDOM, **KW), out, starts=starts, flags=flags, augment=_nat_cfg(aug))
    torch.cuda.synchronize()
    g.check()
    assert flags.tolist() == [0] * C.N_TRACKS + [R.FLAG_BAD_ROW] * 3
    assert not out[C.N_TRACKS:].view(INT[out.dtype]).any()
    assert _equal_bits(out[:C.N_TRACKS], _want(dt, odt, aug)[1])
