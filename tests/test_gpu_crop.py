"""dcue_crop_tracks on the GPU against tests/crop_reference.py. The kernel is a copy (with an exact or a
round-to-nearest-even conversion), so every comparison is bit for bit: there is no tolerance.

The store has 37 tracks whose lengths are drawn from crop_reference.LENGTHS (every length at least
once). 37 rows run as 16 parts per row; the larger row counts reach the other launch shapes: 300 rows
(4 parts), 2,100 rows (whole rows, more units than the grid holds: the strided loop)."""
import numpy as np
import pytest
import torch

import crop_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TRACKS = 37
NP_DTYPE = {0: np.float16, 1: np.float32}
TORCH_DTYPE = {0: torch.float16, 1: torch.float32}
MODES = [(R.FIRST, {}), (R.CENTER, {}), (R.GRID, dict(grid_j=0, grid_n=1)), (R.GRID, dict(grid_j=2, grid_n=5)),
         (R.GRID, dict(grid_j=4, grid_n=5)), (R.RANDOM, dict(seed=0, draw=0)), (R.RANDOM, dict(seed=7, draw=2 ** 40)),
         (R.RANDOM, dict(seed=0, draw=R.FACTOR_DRAW0 + 3))]


def _lengths():
    rs = np.random.RandomState(4)
    lengths = np.concatenate([R.LENGTHS, rs.choice(R.LENGTHS, N_TRACKS - len(R.LENGTHS))])
    return rs.permutation(lengths).astype(np.int64)


_STORES, _TABLES = {}, {}


def _store(dt):
    """(host data, host frame_ptr, device data, device frame_ptr) of the store in dtype dt, made once."""
    if dt not in _STORES:
        data, fp = R.make_store(_lengths(), NP_DTYPE[dt], seed=dt)
        _STORES[dt] = (data, fp, torch.from_numpy(data).to(DEV), torch.from_numpy(fp).to(DEV))
    return _STORES[dt]


def _table(dt, odt, mode, kw):
    """The restatement's crop of every track, made once per case and shared."""
    key = (dt, odt, mode, tuple(sorted(kw.items())))
    if key not in _TABLES:
        data, fp = _store(dt)[:2]
        _TABLES[key] = R.crop(data, fp, None, NP_DTYPE[odt], mode, **kw)
    return _TABLES[key]


def _bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return x.view(np.int16 if x.dtype == np.float16 else np.int32)


def _rows(n, seed=1):
    """A permutation of the tracks with repeats, n entries, every track at least once when n allows."""
    rs = np.random.RandomState(seed)
    rows = np.concatenate([rs.permutation(N_TRACKS), rs.randint(0, N_TRACKS, max(n - N_TRACKS, 0))])[:n]
    return rs.permutation(rows).astype(np.int32)


class _Guarded:
    """out, starts and flags with a sentinel row before and after each, and the check that a call left
    the sentinels alone."""

    def __init__(self, n, odt):
        self.out = torch.full((n + 2, R.W, R.N_MELS), 777.0, dtype=TORCH_DTYPE[odt], device=DEV)
        self.starts = torch.full((n + 2,), -12345, dtype=torch.int32, device=DEV)
        self.flags = torch.full((n + 2,), -12345, dtype=torch.int32, device=DEV)

    def views(self):
        return self.out[1:-1], self.starts[1:-1], self.flags[1:-1]

    def check(self):
        assert bool((self.out[0] == 777.0).all()) and bool((self.out[-1] == 777.0).all())
        assert self.starts[0].item() == self.starts[-1].item() == -12345
        assert self.flags[0].item() == self.flags[-1].item() == -12345


def _crop(dt, odt, mode, kw, rows, frame_ptr=None):
    """One guarded dcue_crop_tracks call: (out, starts, flags) as numpy."""
    from dcrecommend import _native as nat
    _, _, data, fp = _store(dt)
    n = N_TRACKS if rows is None else len(rows)
    g = _Guarded(n, odt)
    out, starts, flags = g.views()
    r = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(DEV)
    nat.crop_tracks(data, fp if frame_ptr is None else frame_ptr, nat.crop_config(mode, **kw), out, rows=r,
                    starts=starts, flags=flags)
    torch.cuda.synchronize()
    g.check()
    return out.cpu().numpy(), starts.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("dt,odt", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_rows_and_starts_equal_the_restatement(dt, odt, with_rows):
    lengths = _lengths()
    rows = _rows(50) if with_rows else None
    sel = np.arange(N_TRACKS) if rows is None else rows
    for mode, kw in MODES:
        want, want_starts, _ = _table(dt, odt, mode, kw)
        out, starts, flags = _crop(dt, odt, mode, kw, rows)
        assert not flags.any()
        assert np.array_equal(starts, want_starts[sel]), (mode, kw)
        assert np.array_equal(_bits(out), _bits(want[sel])), (mode, kw)
        # the tail rows of short tracks are exactly zero (bit pattern 0: no negative zero either)
        for i, t in enumerate(sel):
            assert not _bits(out[i, min(lengths[t], R.W):]).any()
        # the same track gives the same row in any position
        if rows is not None:
            first = {}
            for i, t in enumerate(rows):
                j = first.setdefault(int(t), i)
                assert np.array_equal(_bits(out[i]), _bits(out[j]))
    if dt == 1 and odt == 0:  # the store's ties round to even, its largest value stays finite
        x = _store(1)[0][0, :4]
        assert np.array_equal(x.astype(np.float16), np.array([1.0, 1.0 + 2.0 ** -9, -1.0, 65504.0], dtype=np.float16))
        t0 = int(np.flatnonzero(lengths > 0)[0])  # the track that holds the store's first frame
        out, _, _ = _crop(1, 0, R.FIRST, {}, [t0])
        assert np.array_equal(_bits(out[0, 0, :4]), _bits(x.astype(np.float16)))


@pytest.mark.parametrize("dt,odt,n", [(0, 0, 2100), (0, 0, 600), (1, 0, 300), (0, 1, 300), (0, 0, 150), (1, 1, 70)])
def test_other_launch_shapes(dt, odt, n):
    """More rows than tracks: 1, 2, 4, 8 and 16 parts per row; at 2,100 rows whole rows on a grid
    smaller than the work."""
    mode, kw = R.RANDOM, dict(seed=5, draw=9)
    want, want_starts, _ = _table(dt, odt, mode, kw)
    rows = _rows(n, seed=n)
    out, starts, flags = _crop(dt, odt, mode, kw, rows)
    assert not flags.any() and np.array_equal(starts, want_starts[rows])
    assert np.array_equal(_bits(out), _bits(want[rows]))


@pytest.mark.parametrize("dt,odt", [(0, 0), (1, 0)])
def test_one_call_equals_two_over_a_split(dt, odt):
    mode, kw = R.RANDOM, dict(seed=2, draw=1)
    rows = _rows(50, seed=3)
    whole = _crop(dt, odt, mode, kw, rows)
    for cut in (1, 13, 49):
        a, b = _crop(dt, odt, mode, kw, rows[:cut]), _crop(dt, odt, mode, kw, rows[cut:])
        assert np.array_equal(_bits(whole[0]), np.concatenate([_bits(a[0]), _bits(b[0])]))
        for w, x, y in zip(whole[1:], a[1:], b[1:]):
            assert np.array_equal(w, np.concatenate([x, y]))
    # without rows the output row is the track: rows = 0..n-1 gives the same table
    plain = _crop(dt, odt, mode, kw, None)
    ident = _crop(dt, odt, mode, kw, np.arange(N_TRACKS))
    assert np.array_equal(_bits(plain[0]), _bits(ident[0])) and np.array_equal(plain[1], ident[1])


@pytest.mark.parametrize("dt,odt", [(0, 0), (1, 1), (0, 1)])
def test_corrupt_extents_and_rows_are_flagged_and_zero(dt, odt):
    """One frame_ptr entry and one rows entry corrupted: those rows come back flagged and zero, every
    other row unchanged, nothing outside `out` written. The last frame_ptr entry reaches past the store
    (one track); a negative entry in the middle makes two extents bad (the track it ends, the one it starts)."""
    mode, kw = R.RANDOM, dict(seed=0, draw=4)
    data, fp_host, _, _ = _store(dt)
    rows = _rows(50, seed=8)
    clean = _crop(dt, odt, mode, kw, rows)
    for entry, value, bad_tracks in ((N_TRACKS, len(data) + 5, {N_TRACKS - 1}), (11, -3, {10, 11})):
        for bad_row_value in (N_TRACKS, -1, 2 ** 31 - 1):
            fp = fp_host.copy()
            fp[entry] = value
            r = rows.copy()
            victim = int(np.flatnonzero(~np.isin(rows, list(bad_tracks)))[5])
            r[victim] = bad_row_value
            want, want_starts, want_flags = R.crop(data, fp, r, NP_DTYPE[odt], mode, total_frames=len(data), **kw)
            out, starts, flags = _crop(dt, odt, mode, kw, r, frame_ptr=torch.from_numpy(fp).to(DEV))
            assert np.array_equal(flags, want_flags)
            hit = np.isin(rows, list(bad_tracks))
            assert hit.any() and np.all(flags[hit] == R.FLAG_BAD_EXTENT) and flags[victim] == R.FLAG_BAD_ROW
            flagged = hit.copy()
            flagged[victim] = True
            assert not flags[~flagged].any()
            assert not _bits(out[flagged]).any() and not starts[flagged].any()
            assert np.array_equal(_bits(out[~flagged]), _bits(clean[0][~flagged]))
            assert np.array_equal(starts[~flagged], clean[1][~flagged])
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(starts, want_starts)
    # without rows, an output row past the last track is a bad row
    from dcrecommend import _native as nat
    _, _, ddata, dfp = _store(dt)
    g = _Guarded(N_TRACKS + 3, odt)
    out, starts, flags = g.views()
    nat.crop_tracks(ddata, dfp, nat.crop_config(mode, **kw), out, starts=starts, flags=flags)
    torch.cuda.synchronize()
    g.check()
    assert flags.tolist() == [0] * N_TRACKS + [R.FLAG_BAD_ROW] * 3
    assert not out[N_TRACKS:].any() and np.array_equal(_bits(out[:N_TRACKS]), _bits(_crop(dt, odt, mode, kw, None)[0]))


def test_flags_of_an_earlier_call_do_not_linger_and_starts_are_optional():
    from dcrecommend import _native as nat
    _, _, data, fp = _store(0)
    out = torch.empty((4, R.W, R.N_MELS), dtype=torch.float16, device=DEV)
    flags = torch.full((4,), 3, dtype=torch.int32, device=DEV)
    rows = torch.tensor([0, 99, 2, 3], dtype=torch.int32, device=DEV)
    nat.crop_tracks(data, fp, nat.crop_config(nat.CROP_CENTER), out, rows=rows, flags=flags)
    assert flags.tolist() == [0, R.FLAG_BAD_ROW, 0, 0]
    rows[1] = 1
    nat.crop_tracks(data, fp, nat.crop_config(nat.CROP_CENTER), out, rows=rows, flags=flags)
    assert flags.tolist() == [0, 0, 0, 0]
    want = _table(0, 0, R.CENTER, {})[0][[0, 1, 2, 3]]
    assert np.array_equal(_bits(out), _bits(want))
