"""The cases tests/test_gpu_rank_regimes.py runs dcue_rank_metrics at, against oracle/rank_oracle.py,
and the regime facts each case promises (tests/test_rank_regimes_cpu.py checks them from the inputs
alone, so a seed or class mix that drifts fails on the CPU). No GPU is touched at import.

Every case has exactly representable scores: a factor row has m entries of +-1 at random positions
(m = 16 for d >= 16, 4 for 4 <= d < 16, 1 for d < 4: norms 4, 2, 1), so a cosine is a multiple of 1/m,
exact in fp32 under any summation order, and GPU and oracle are held to 1e-12.

A CSR row is built with an exact number n of positives inside the mode's lists (mode 0: a candidate of
either list; mode 1: a bit-1 candidate) plus entries that do not count (class 0; in mode 1 also the
bit-0-only candidates), so n is a promise of the case, not a draw.
"""
import collections
import functools

import numpy as np

from oracle import rank_oracle as R

CAP = 4096     # kRankCap: positives inside the lists per query
CHUNK = 8192   # kRankChunk: candidates per histogram workgroup
TILE = 64      # kRankTile: queries per scoring workgroup
P_CLASS = [0.1, 0.3, 0.5, 0.1]

Case = collections.namedtuple("Case", "name qf cand inp queries mode qb direct facts")
# facts: row_n [n_rows] promised in-list positives per CSR row; n_set (optional) the exact set of n
# over the queried rows; chunks, last_chunk; passes (sizes); runs {row: its longest run of equal
# thresholds is at least this}; further case-specific entries.


def weight(d):
    return 16 if d >= 16 else 4 if d >= 4 else 1


def lattice(rs, n, d):
    """n rows with weight(d) entries of +-1 at random positions, zeros elsewhere."""
    m = weight(d)
    x = np.zeros((n, d), np.float32)
    pos = np.argsort(rs.rand(n, d), axis=1)[:, :m]
    np.put_along_axis(x, pos, rs.choice(np.array([-1.0, 1.0], np.float32), (n, m)), axis=1)
    return x


def sprinkle(rs, cand):
    """test_gpu_eval's sprinklings: 5 % duplicated rows (exact ties), three all-zero rows."""
    n = len(cand)
    dup = rs.choice(n, n // 20, replace=False)
    cand[dup] = cand[rs.choice(n, len(dup))]
    cand[rs.choice(n, min(3, n // 16), replace=False)] = 0.0
    return cand


def draw_classes(rs, n_cand):
    """The class mix of test_gpu_eval; the candidates at a histogram chunk's edges (the last of the first
    chunk, the first of the second, the last of all) are in both lists, so every mode counts them."""
    cls = rs.choice(np.array([0, 1, 2, 3], np.uint8), n_cand, p=P_CLASS)
    cls[-1] = 3
    if n_cand > CHUNK:
        cls[CHUNK - 1] = cls[CHUNK] = 3
    return cls


def count_mask(cls, mode):
    """The candidates that count as a query's positive when its CSR row lists them."""
    cls = np.asarray(cls)
    return cls != 0 if mode == 0 else (cls & 2) != 0


def csr_exact(rs, cls, mode, ns, extras):
    """CSR rows with exactly ns[r] counting candidates and up to extras[r] that do not count."""
    counted = np.flatnonzero(count_mask(cls, mode))
    other = np.flatnonzero(~count_mask(cls, mode))
    ptr, idx = [0], []
    for n, x in zip(ns, extras):
        x = min(x, len(other))
        row = np.concatenate([rs.choice(counted, n, replace=False) if n else counted[:0],
                              rs.choice(other, x, replace=False) if x else other[:0]])
        idx.append(np.sort(row))
        ptr.append(ptr[-1] + len(row))
    return {"pos_ptr": np.array(ptr, np.int64), "pos_idx": np.concatenate(idx).astype(np.int32),
            "cand_class": np.asarray(cls, np.uint8)}


def passes(nq, qb):
    return [min(qb, nq - q0) for q0 in range(0, nq, qb)]


def _facts(n_cand, d, nq, qb, row_n, **more):
    f = {"row_n": np.asarray(row_n), "d": d, "chunks": -(-n_cand // CHUNK),
         "last_chunk": n_cand - (-(-n_cand // CHUNK) - 1) * CHUNK, "passes": passes(nq, qb), "runs": {}}
    f.update(more)
    return f


def _random_ns(rs, n_rows, cls, mode, max_pos):
    """Row 0 has no positive, row 1 as many as max_pos and the lists allow, the rest anything between;
    a row's entries (extras included) stay within max_pos."""
    avail = int(count_mask(cls, mode).sum())
    hi = min(max_pos, avail)
    ns = [0, hi] + [int(rs.randint(0, hi + 1)) for _ in range(n_rows - 2)]
    extras = [int(rs.randint(0, min(20, max_pos - n) + 1)) for n in ns]
    return ns[:n_rows], extras[:n_rows], hi


# --- threshold count and cap -----------------------------------------------------------------
THRESHOLD_NS = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1024, 4095, 4096]
THRESHOLD_QB = 16


@functools.lru_cache(maxsize=None)
def _threshold_data(mode):
    """n_cand = 9,001 (two chunks, the second ragged), d = 32; row r < 12 has n = THRESHOLD_NS[r], row
    12 has n = 4,096 among more than 4,096 entries, row 13 is over the cap (n = 4,097)."""
    rs = np.random.RandomState(100 + mode)
    n_cand, d = 9001, 32
    cand = sprinkle(rs, lattice(rs, n_cand, d))
    cls = draw_classes(rs, n_cand)
    ns = THRESHOLD_NS + [CAP, CAP + 1]
    extras = [int(rs.randint(1, 100)) for _ in ns]
    extras[12] = 300
    inp = csr_exact(rs, cls, mode, ns, extras)
    return lattice(rs, len(ns), d), cand, inp, ns


def threshold_case(mode):
    qf, cand, inp, ns = _threshold_data(mode)
    rs = np.random.RandomState(7)
    queries = np.concatenate([rs.permutation(13), rs.choice(13, 6, replace=False)]).astype(np.int32)
    return Case("threshold-m%d" % mode, qf, cand, inp, queries, mode, THRESHOLD_QB, False,
                _facts(9001, 32, len(queries), THRESHOLD_QB, ns, n_set=set(THRESHOLD_NS), runs={12: 512}))


CAP_PLACES = {"first": 0, "mid": 5, "second": THRESHOLD_QB + 1}


def cap_case(mode, place):
    """threshold_case's data; facts["bad_queries"] has the over-cap row at position CAP_PLACES[place]:
    the first query of the first pass, a later one of it, or one of the second pass."""
    c = threshold_case(mode)
    bad = c.queries.copy()
    bad[CAP_PLACES[place]] = 13
    f = dict(c.facts, bad_queries=bad, bad_at=CAP_PLACES[place])
    return c._replace(name="cap-%s-m%d" % (place, mode), facts=f)


# --- the general builder -----------------------------------------------------------------------
def _general(name, seed, mode, n_rows, n_cand, d, max_pos, nq, qb, direct=False, cls=None, **more):
    rs = np.random.RandomState(seed)
    cand = sprinkle(rs, lattice(rs, n_cand, d))
    if cls is None:
        cls = draw_classes(rs, n_cand)
    ns, extras, hi = _random_ns(rs, n_rows, cls, mode, max_pos)
    inp = csr_exact(rs, cls, mode, ns, extras)
    qf = lattice(rs, n_rows, d)
    queries = rs.randint(0, n_rows, nq).astype(np.int32)
    queries[:2] = [1, 0]  # the fullest and the empty row are always asked
    return Case(name, qf, cand, inp, queries, mode, qb, direct,
                _facts(n_cand, d, nq, qb, ns, n_max=hi, **more))


CAND_COUNTS = [1, 63, 64, 65, 8191, 8192, 8193, 20001]


def cand_case(mode, n_cand):
    """d = 16, 40 rows, rows of up to min(300, n_cand) entries, one pass of 60 queries. n_cand = 1: the
    candidate is in both lists and is the positive of every odd row."""
    name = "cand%d-m%d" % (n_cand, mode)
    if n_cand > 1:
        return _general(name, 200 + n_cand % 97 + mode, mode, 40, n_cand, 16, min(300, n_cand), 60, 60)
    rs = np.random.RandomState(200 + mode)
    ns = [r & 1 for r in range(40)]
    inp = csr_exact(rs, np.array([3], np.uint8), mode, ns, [0] * 40)
    queries = rs.randint(0, 40, 60).astype(np.int32)
    queries[:2] = [1, 0]
    return Case(name, lattice(rs, 40, 16), lattice(rs, 1, 16), inp, queries, mode, 60, False,
                _facts(1, 16, 60, 60, ns, n_max=1))


PASS_QBS = [1, 5, 16, 63, 64, 65, 128, 257, 300, 1000]
PASS_DIRECT = (1, 5)  # below the binding's floor of 16: through the C entry point


@functools.lru_cache(maxsize=None)
def _pass_data(mode, gaussian):
    c = _general("pass", 300 + mode, mode, 150, 8193, 100, 150, 300, 300)
    if gaussian:
        rs = np.random.RandomState(310 + mode)
        c = c._replace(qf=rs.randn(150, 100).astype(np.float32),
                       cand=sprinkle(rs, rs.randn(8193, 100).astype(np.float32)))
    return c


def pass_case(mode, qb, gaussian=False):
    """n_cand = 8,193 (two chunks, the second of one candidate), d = 100, 300 queries over 150 rows,
    query_batch = qb. The binding caps qb at the number of queries, so 1,000 runs as one pass of 300."""
    c = _pass_data(mode, gaussian)
    eff = min(qb, len(c.queries)) if qb not in PASS_DIRECT else qb
    f = dict(c.facts, passes=passes(len(c.queries), eff), gaussian=gaussian)
    return c._replace(name="pass%d%s-m%d" % (qb, "-gauss" if gaussian else "", mode), qb=qb,
                      direct=qb in PASS_DIRECT, facts=f)


WIDTHS = [1, 2, 3, 4, 7, 15, 16, 17, 20, 255, 256]


def width_case(mode, d):
    """test_rank_metrics_lattice_exact's shape (2,500 candidates, 120 rows, up to 150 positives, 150
    queries in passes of 64) at the widths it does not run."""
    return _general("width%d-m%d" % (d, mode), 400 + d + mode, mode, 120, 2500, d, 150, 150, 64)


# --- tie structure ---------------------------------------------------------------------------
def identical_case(mode, d):
    """Every candidate row is the same vector: all of a query's scores tie, and the AUC of a set with
    both labels is exactly 0.5."""
    c = _general("identical-d%d-m%d" % (d, mode), 500 + d + mode, mode, 40, 2500, d, 300, 60, 60)
    cand = np.repeat(lattice(np.random.RandomState(501), 1, d), 2500, axis=0)
    return c._replace(cand=cand, facts=dict(c.facts, runs={1: c.facts["n_max"]}, all_tie=True))


TIE_NS = [0, 1, 600, 2500, 4000]


def tie_case(mode):
    """d = 1: a score is -1, 0 or +1, so a row with n positives has two threshold runs of about n / 2:
    longer than 256 (n = 600) and than 1,024 (n = 2,500 and 4,000), each spanning many of the scan's
    per-thread segments and of the finalize loop's 256-strides. 8,000 candidates, one chunk."""
    rs = np.random.RandomState(600 + mode)
    n_cand = 8000
    cand = sprinkle(rs, lattice(rs, n_cand, 1))
    cls = draw_classes(rs, n_cand)
    ns = TIE_NS + [int(rs.randint(0, 301)) for _ in range(15)]
    inp = csr_exact(rs, cls, mode, ns, [int(rs.randint(0, 50)) for _ in ns])
    queries = np.concatenate([np.arange(20), rs.randint(0, 20, 10)]).astype(np.int32)
    return Case("tie-d1-m%d" % mode, lattice(rs, 20, 1), cand, inp, queries, mode, 30, False,
                _facts(n_cand, 1, 30, 30, ns, runs={2: 257, 3: 1025, 4: 1025}))


# --- degenerate lists ------------------------------------------------------------------------
DEGENERATE = ("nobit0", "nobit1", "allpos")


def degenerate_case(mode, kind):
    """600 candidates, d = 16, 30 rows. nobit0 / nobit1: no candidate carries that list bit. allpos:
    row 0 lists every candidate of a list (each list item is the query's positive); row 1's positives
    are in the other list only (mode 0: no pred positive, has_pos = 0) and is asked in the middle of the
    sample, ordinary queries after it."""
    rs = np.random.RandomState(700 + mode + 10 * DEGENERATE.index(kind))
    n_cand, d, n_rows = 600, 16, 30
    cls = {"nobit0": rs.choice(np.array([0, 2], np.uint8), n_cand, p=[0.2, 0.8]),
           "nobit1": rs.choice(np.array([0, 1], np.uint8), n_cand, p=[0.2, 0.8]),
           "allpos": rs.choice(np.array([0, 1, 2, 3], np.uint8), n_cand, p=P_CLASS)}[kind]
    c = _general("degenerate-%s-m%d" % (kind, mode), 710 + mode, mode, n_rows, n_cand, d, 150, 40, 16, cls=cls)
    if kind != "allpos":
        return c
    ptr, idx = c.inp["pos_ptr"], c.inp["pos_idx"]
    rows = [idx[ptr[r]:ptr[r + 1]] for r in range(n_rows)]
    rows[0] = np.flatnonzero(cls != 0).astype(np.int32)
    other_list = 2 if mode == 0 else 1
    rows[1] = np.flatnonzero(cls == other_list)[:40].astype(np.int32)
    ns = c.facts["row_n"].copy()
    ns[0] = int(count_mask(cls, mode).sum())
    ns[1] = 40 if mode == 0 else 0
    inp = {"pos_ptr": np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
           "pos_idx": np.concatenate(rows).astype(np.int32), "cand_class": cls}
    queries = c.queries.copy()
    queries[np.isin(queries, [0, 1])] = 9
    queries[:2] = [5, 6]
    queries[18:22] = [0, 1, 7, 0]
    return c._replace(inp=inp, queries=queries,
                      facts=dict({k: v for k, v in c.facts.items() if k != "n_max"}, row_n=ns, all_pos_row=0,
                                 other_list_row=1))


# --- non-finite factors at scale ---------------------------------------------------------------
NONFINITE_NAN_AT = 70  # position of the NaN query: first pass, second query tile


def nonfinite_case(mode):
    """n_cand = 20,001 (three chunks, the last of 3,617), d = 128, 200 queries in passes of 128 and 72.
    Rows 2.. have 20 to 300 positives; row 0 is asked only at position NONFINITE_NAN_AT; row 1 (its
    positives are in the truth list only) is not asked in the clean run."""
    rs = np.random.RandomState(800 + mode)
    n_cand, d, n_rows, nq, qb = 20001, 128, 60, 200, 128
    cand = sprinkle(rs, lattice(rs, n_cand, d))
    cls = draw_classes(rs, n_cand)
    ns = [int(rs.randint(20, 301)) for _ in range(n_rows)]
    inp = csr_exact(rs, cls, mode, ns, [int(rs.randint(0, 20)) for _ in ns])
    ptr, idx = inp["pos_ptr"], inp["pos_idx"]
    rows = [idx[ptr[r]:ptr[r + 1]] for r in range(n_rows)]
    rows[1] = np.flatnonzero(cls == 2)[:30].astype(np.int32)
    ns[1] = 30
    inp = {"pos_ptr": np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
           "pos_idx": np.concatenate(rows).astype(np.int32), "cand_class": cls}
    queries = rs.randint(2, n_rows, nq).astype(np.int32)
    queries[NONFINITE_NAN_AT] = 0
    return Case("nonfinite-m%d" % mode, lattice(rs, n_rows, d), cand, inp, queries, mode, qb, False,
                _facts(n_cand, d, nq, qb, ns, nan_row=0, no_pred_row=1))


def nonfinite_variants(c):
    """(name, query_feat, cand_feat, queries, raises, same_as_clean, oracle's queries) of a
    nonfinite_case. The oracle is asked only as many leading queries as decide whether it raises."""
    cls = c.inp["cand_class"]
    out = []
    bad = c.cand.copy()  # (a) a label-0 / pred-list candidate of the second chunk
    bad[CHUNK + int(np.flatnonzero(cls[CHUNK:] & 1)[0])] = np.nan
    out.append(("listed-candidate", c.qf, bad, c.queries, True, False, c.queries[:4]))
    outside = c.cand.copy()  # (b) candidates of no list, in the second and the ragged last chunk
    free = np.flatnonzero(cls == 0)
    outside[free[(free >= CHUNK) & (free < 2 * CHUNK)][:5]] = np.nan
    outside[free[free >= 2 * CHUNK][:5]] = np.nan
    outside[free[-1]] = np.nan
    out.append(("unlisted-candidates", c.qf, outside, c.queries, False, True, c.queries[:8]))
    nanq = c.qf.copy()  # (c) the query at position 70 of the first pass
    nanq[c.facts["nan_row"]] = np.nan
    out.append(("query", nanq, c.cand, c.queries, True, False, c.queries[:NONFINITE_NAN_AT + 1]))
    if c.mode == 0:  # ... after a query without pred positives: the reference's loop has ended
        late = c.queries.copy()
        late[10] = c.facts["no_pred_row"]
        out.append(("query-after-break", nanq, c.cand, late, False, False, late[:NONFINITE_NAN_AT + 1]))
    return out


# --- registry --------------------------------------------------------------------------------
def _registry():
    entries = [(threshold_case, ())]
    entries += [(cand_case, (n,)) for n in CAND_COUNTS]
    entries += [(pass_case, (qb,)) for qb in PASS_QBS]
    entries += [(width_case, (d,)) for d in WIDTHS]
    entries += [(identical_case, (d,)) for d in (1, 16)]
    entries += [(tie_case, ())]
    entries += [(degenerate_case, (k,)) for k in DEGENERATE]
    entries += [(nonfinite_case, ())]
    return [(fn, mode, args) for fn, args in entries for mode in (0, 1)]


_ENTRIES = _registry()


def _name(fn, mode, args):
    stem = {threshold_case: "threshold", cand_case: "cand%d", pass_case: "pass%d", width_case: "width%d",
            identical_case: "identical-d%d", tie_case: "tie-d1", degenerate_case: "degenerate-%s",
            nonfinite_case: "nonfinite"}[fn]
    return (stem % args if args else stem) + "-m%d" % mode


# name -> (builder, mode, args): every case the GPU test holds to the oracle (the cap placements and
# the gaussian batching variant are asked for by name: cap_case, pass_case(gaussian=True))
CASES = collections.OrderedDict((_name(*e), e) for e in _ENTRIES)


@functools.lru_cache(maxsize=None)
def get(name):
    fn, mode, args = CASES[name]
    c = fn(mode, *args)
    assert c.name == name, (c.name, name)
    return c


# --- what the CPU test measures from the inputs alone -------------------------------------------------
def in_list_positives(c):
    """n per CSR row, counted from the inputs."""
    ptr, idx = c.inp["pos_ptr"], c.inp["pos_idx"]
    counts = count_mask(c.inp["cand_class"], c.mode)
    return np.array([int(counts[idx[ptr[r]:ptr[r + 1]]].sum()) for r in range(len(ptr) - 1)])


def longest_threshold_run(c, row):
    """The longest run of equal thresholds of a CSR row, from the oracle's scores (torch's fp32 cosine)."""
    ptr, idx = c.inp["pos_ptr"], c.inp["pos_idx"]
    mine = idx[ptr[row]:ptr[row + 1]]
    mine = mine[count_mask(c.inp["cand_class"], c.mode)[mine]]
    if not len(mine):
        return 0
    s = R.cosine_rows(np.repeat(c.qf[row:row + 1], len(mine), axis=0), c.cand[mine])
    return int(np.unique(s, return_counts=True)[1].max())


def restated_metrics(c):
    """R.rank_metrics with the scores restated in integers: cand @ q / m in fp64 (rows have m entries of
    +-1 or are zero, so that is the cosine exactly), through the same user_metrics / song_metrics."""
    cls = c.inp["cand_class"]
    ptr, idx = c.inp["pos_ptr"], c.inp["pos_idx"]
    inP, inT = (cls & 1) != 0, (cls & 2) != 0
    C, Q, m = c.cand.astype(np.float64), c.qf.astype(np.float64), weight(c.cand.shape[1])
    auc, ap = np.zeros(len(c.queries)), np.zeros(len(c.queries))
    flag = np.zeros(len(c.queries), np.int32)
    for k, q in enumerate(c.queries):
        pos = np.zeros(len(cls), bool)
        pos[idx[ptr[q]:ptr[q + 1]]] = True
        s = C @ Q[q] / m
        if c.mode == 0:
            flag[k] = int((pos & inP).any())
            auc[k], ap[k] = R.user_metrics(s[inP], pos[inP].astype(int), s[inT], pos[inT].astype(int))
        else:
            sp = s[pos & inT]
            flag[k] = int(len(sp) > 0)
            auc[k], ap[k] = R.song_metrics(np.concatenate([sp, s[inP]]),
                                           np.concatenate([np.ones(len(sp), int), np.zeros(int(inP.sum()), int)]))
    return auc, ap, flag


def oracle_of(c):
    """R.rank_metrics of a case, read-only."""
    out = R.rank_metrics(c.qf, c.cand, c.queries, c.inp["pos_ptr"], c.inp["pos_idx"], c.inp["cand_class"], c.mode)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle_of(get(name))


def oracle(name):
    """oracle_of a registered case, computed once per process and shared: the queries-per-pass cases
    of a mode are one problem under ten batchings, so they share one result."""
    c = get(name)
    return _oracle("pass%d-m%d" % (PASS_QBS[0], c.mode) if name.startswith("pass") else name)
