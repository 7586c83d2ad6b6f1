"""Host side of the hard negatives (include/dcue.h dcue_select_negatives, added under ABI 17), no GPU
needed: the numpy reference against a brute-force restatement and hand cases, the ABI, the refusals
before any device call, DCUE's arguments, the train script's flags and the kernel's resources."""
import ctypes
import os
import re

import numpy as np
import pytest

import hard_negatives_reference as R
from kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------------------------- reference
def _brute(user_feat, item_feat, users, pool, N, H):
    """The definition restated with plain loops: no argsort, no unique, no setdiff."""
    out, hard, flags = [], [], []
    for b, row in enumerate(pool):
        u = int(users[b])
        if not 0 <= u < len(user_feat):
            out.append([int(x) for x in row[:N]])
            hard.append(0)
            flags.append(2)
            continue
        uf = [float(x) for x in user_feat[u]]
        un = max(sum(x * x for x in uf) ** 0.5, 1e-8)
        flag, cands, seen = 0, [], set()
        for p, i in enumerate(int(x) for x in row):
            if not 0 <= i < len(item_feat):
                flag |= 2
                continue
            c = [float(x) for x in item_feat[i]]
            cn = max(sum(x * x for x in c) ** 0.5, 1e-8)
            s = sum(x * y for x, y in zip(uf, c)) / (un * cn)
            if s != s or s in (float("inf"), float("-inf")):
                flag |= 1
            if i not in seen and s == s:
                cands.append((s, p))
            seen.add(i)
        chosen = []
        while len(chosen) < H and cands:  # the best left: highest score, then earliest position
            best = cands[0]
            for c in cands[1:]:
                if c[0] > best[0] or (c[0] == best[0] and c[1] < best[1]):
                    best = c
            cands.remove(best)
            chosen.append(best[1])
        chosen.sort()
        rest = [p for p in range(len(row)) if p not in chosen][:N - len(chosen)]
        out.append([int(row[p]) for p in chosen + rest])
        hard.append(len(chosen))
        flags.append(flag)
    return np.array(out, dtype=np.int64), np.array(hard, dtype=np.int32), np.array(flags, dtype=np.int32)


@pytest.mark.parametrize("d,P,N,H", [(1, 1, 1, 1), (3, 7, 4, 2), (30, 21, 20, 10), (100, 67, 20, 20), (8, 12, 12, 12),
                                     (8, 40, 5, 0)])
def test_reference_equals_the_brute_force(d, P, N, H):
    rs = np.random.RandomState(d + P)
    n_items, n_users, n = 25, 6, 40
    uf = rs.randn(n_users, d).astype(np.float32)
    itf = rs.randn(n_items, d).astype(np.float32)
    itf[3] = itf[11]          # two ids with one row: an exact tie
    itf[5, 0] = NAN
    uf[2] = 0
    pool = rs.randint(-1, n_items + 2, (n, P)).astype(np.int64)  # duplicates, -1 and two ids past the table
    users = rs.randint(0, n_users, n).astype(np.int64)
    users[7], users[8] = -1, n_users
    got, want = R.select(uf, itf, users, pool, N, H), _brute(uf, itf, users, pool, N, H)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[0].shape == (n, N) and got[0].dtype == np.int64


def _one(uf, itf, pool, N, H, user=0):
    out, hard, flags = R.select(np.asarray(uf, np.float32), np.asarray(itf, np.float32), [user], [pool], N, H)
    return out[0].tolist(), int(hard[0]), int(flags[0])


def test_reference_hand_cases():
    uf = [[1.0, 0.0]]
    #          0: cos 1   1: cos 0   2: cos -1   3: cos 0.6   4: = item 0   5: NaN row
    itf = [[2.0, 0.0], [0.0, 3.0], [-1.0, 0.0], [3.0, 4.0], [2.0, 0.0], [NAN, 1.0]]
    # best two of {1, 3, 2}: item 3 (0.6) and item 1 (0), kept in pool order; then the leading others
    assert _one(uf, itf, [1, 3, 2, 1], 3, 2) == ([1, 3, 2], 2, 0)
    # duplicates: only the first occurrence of item 0 can be hard, the second passes through the fill
    assert _one(uf, itf, [2, 0, 0, 3], 4, 2) == ([0, 3, 2, 0], 2, 0)
    # bitwise-equal rows under two ids tie: the earlier position wins
    assert _one(uf, itf, [4, 0, 2], 2, 1) == ([4, 0], 1, 0)
    assert _one(uf, itf, [0, 4, 2], 2, 1) == ([0, 4], 1, 0)
    # NaN: never hard, bit 1
    assert _one(uf, itf, [5, 2, 1], 2, 2) == ([2, 1], 2, 1)
    assert _one(uf, itf, [5, 5], 2, 2) == ([5, 5], 0, 1)
    # -1 and an id past the table: never hard, bit 2, copied through the fill
    assert _one(uf, itf, [-1, 6, 2, 1], 4, 2) == ([2, 1, -1, 6], 2, 2)
    assert _one(uf, itf, [-1, 6, 2, 1], 3, 1) == ([1, -1, 6], 1, 2)
    # fewer than H distinct ids
    assert _one(uf, itf, [2, 2, 2, 2], 3, 3) == ([2, 2, 2], 1, 0)
    assert _one(uf, itf, [-1, -1], 2, 2) == ([-1, -1], 0, 2)
    # H = 0: the plain draws
    assert _one(uf, itf, [3, 0, 1, 2], 2, 0) == ([3, 0], 0, 0)
    # P = N = H: every distinct id is hard, the rest follow
    assert _one(uf, itf, [2, 1, 2, 0], 4, 4) == ([2, 1, 0, 2], 3, 0)
    assert _one(uf, itf, [2, 1, 3, 0], 4, 4) == ([2, 1, 3, 0], 4, 0)
    # a zero user row: every score 0, the first h first occurrences
    assert _one([[0.0, 0.0]], itf, [2, 2, 0, 3, 1], 3, 2) == ([2, 0, 2], 2, 0)
    # a user id outside the table: bit 2 and the plain draws
    assert _one(uf, itf, [3, 0, 1], 2, 2, user=1) == ([3, 0], 0, 2)
    assert _one(uf, itf, [3, 0, 1], 2, 2, user=-1) == ([3, 0], 0, 2)


def test_check_against_accepts_the_definition_and_nothing_far_from_it():
    rs = np.random.RandomState(3)
    uf, itf = rs.randn(5, 16).astype(np.float32), rs.randn(60, 16).astype(np.float32)
    pool = rs.randint(0, 60, (30, 24)).astype(np.int64)
    users = rs.randint(0, 5, 30).astype(np.int64)
    out, hard, _ = R.select(uf, itf, users, pool, 10, 4)
    assert R.check_against(uf, itf, users, pool, 10, 4, out, hard) == 30
    s, _, elig = R.row_scores(uf, itf, users[0], pool[0])
    worst = np.flatnonzero(elig)[np.argmin(s[elig])]  # far below the boundary: swapping it in must fail
    order = np.flatnonzero(elig)[np.argsort(-s[elig], kind="stable")]
    bad = out.copy()
    bad[0] = R.fill(pool[0], np.append(order[:3], worst), 10)
    with pytest.raises(AssertionError):
        R.check_against(uf, itf, users, pool, 10, 4, bad, hard)
    with pytest.raises(AssertionError):
        R.check_against(uf, itf, users, pool, 10, 4, out, hard - 1)
    assert R.tau(100) == 400 * 2.0 ** -24 and R.tau(1) == 128 * 2.0 ** -24


# ------------------------------------------------------------------------------------- ABI
def test_abi():
    from dcrecommend import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dcue.h")).read()
    assert re.search(r"\bint dcue_select_negatives\(", hdr)
    assert re.search(r"#define DCUE_SELECT_MAX_POOL 1024\b", hdr)
    assert "(added under ABI 17) Hard negatives" in hdr
    assert re.search(r"#define DCUE_ABI_VERSION 17\b", hdr)
    assert "dcue_select_negatives" in nat._SIGS and len(nat._SIGS["dcue_select_negatives"][0]) == 15
    assert nat.SELECT_MAX_POOL == 1024 and (nat.SELECT_FLAG_NONFINITE, nat.SELECT_FLAG_BAD_ID) == (1, 2)
    lib = nat.lib()
    assert lib.dcue_select_negatives.argtypes == nat._SIGS["dcue_select_negatives"][0]
    assert lib.dcue_abi_version() == nat.ABI_VERSION == 17


def test_refusals_come_before_any_device_call():
    """Without a GPU a device call would return DCUE_ERR_HIP; every refusal returns its own status, and
    the launch counter stands still."""
    from dcrecommend import _native as nat
    lib = nat.lib()
    OK, INVALID, UNSUPPORTED = 0, 1, nat.ERR_UNSUPPORTED
    buf = (ctypes.c_int64 * 8)()  # an address that is never read or written here
    A = ctypes.cast(buf, ctypes.c_void_p)

    def call(user_feat=A, n_users=4, item_feat=A, n_items=4, d=8, users=A, pool=A, n_samples=2, P=8, N=4, H=2,
             out=A, out_hard=A, out_flags=A):
        return lib.dcue_select_negatives(user_feat, n_users, item_feat, n_items, d, users, pool, n_samples, P, N, H,
                                         out, out_hard, out_flags, None)

    launches = lib.dcue_launch_count()
    for name in ("user_feat", "item_feat", "users", "pool", "out", "out_hard", "out_flags"):
        assert call(**{name: None}) == INVALID, name
    assert call(N=0) == INVALID and call(N=9) == INVALID                  # 1 <= N <= P
    assert call(P=1025, N=4) == INVALID and call(P=0, N=0) == INVALID     # P <= DCUE_SELECT_MAX_POOL
    assert call(H=-1) == INVALID and call(H=5) == INVALID                 # 0 <= H <= N
    assert call(n_samples=-1) == INVALID
    assert call(d=0) == INVALID and call(d=-3) == INVALID
    assert call(n_users=-1) == INVALID and call(n_items=-1) == INVALID
    assert call(d=257) == UNSUPPORTED
    assert call(d=257, N=0) == INVALID                                    # a violation outranks the width
    assert call(n_samples=0) == OK and call(n_samples=0, d=256, P=1024, N=1024, H=1024) == OK
    assert call(n_samples=0, d=257) == UNSUPPORTED
    assert lib.dcue_launch_count() == launches


# ------------------------------------------------------------------------------------- trainer
def test_dcue_arguments():
    from dcrecommend.nn.dcue import DCUE
    t = DCUE(device="cpu")
    assert t.neg_pool is None and t.neg_hard is None
    assert "neg_pool" in DCUE._SCALARS and "neg_hard" in DCUE._SCALARS
    t = DCUE(device="cpu", neg_pool=160)
    assert (t.neg_pool, t.neg_hard) == (160, None)
    assert DCUE._check_neg_pool(160, None, 20) == (160, 10)   # the default: N // 2
    assert DCUE._check_neg_pool(160, None, 1) == (160, 0)
    assert DCUE._check_neg_pool(20, 0, 20) == (20, 0)
    assert DCUE._check_neg_pool(1024, 20, 20) == (1024, 20)
    assert DCUE._check_neg_pool(None, None, 20) is None
    t = DCUE(device="cpu", neg_pool=np.int64(40), neg_hard=np.int64(7))
    assert (t.neg_pool, t.neg_hard) == (40, 7) and type(t.neg_pool) is int
    for kw in (dict(neg_pool=0), dict(neg_pool=1025), dict(neg_pool=-5), dict(neg_pool=40, neg_hard=-1),
               dict(neg_pool=40, neg_hard=41), dict(neg_hard=3), dict(neg_pool=40.5), dict(neg_pool=True)):
        with pytest.raises(ValueError):
            DCUE(device="cpu", **kw)
    # against N, known at the first train epoch
    for P, H, N in ((19, None, 20), (40, 21, 20)):
        with pytest.raises(ValueError):
            DCUE._check_neg_pool(P, H, N)
    fmt = DCUE(device="cpu", neg_pool=160, neg_hard=5)._format_model_subdir()
    assert fmt == DCUE(device="cpu")._format_model_subdir()


def test_train_dcue_options(capsys):
    import train_dcue
    a = train_dcue.parse(["--synthetic"])
    assert a.neg_pool is None and a.neg_hard is None
    a = train_dcue.parse(["--synthetic", "--neg-pool", "160", "--neg-hard", "5"])
    assert (a.neg_pool, a.neg_hard) == (160, 5)
    a = train_dcue.parse(["--synthetic", "--neg-pool", "20"])
    assert (a.neg_pool, a.neg_hard) == (20, None)
    for bad in (["--neg-hard", "3"], ["--neg-pool", "19"], ["--neg-pool", "1025"], ["--neg-pool", "40", "--neg-hard", "21"],
                ["--neg-pool", "40", "--neg-hard", "-1"], ["--neg-pool", "x"]):
        with pytest.raises(SystemExit):
            train_dcue.parse(["--synthetic"] + bad)
    capsys.readouterr()


# ------------------------------------------------------------------------------------- kernel
def test_kernel_resources(tmp_path):
    res = kernel_resources("hardneg.hip", tmp_path)
    # one instantiation per width class: d <= 32, 64, 128, 256
    assert len(res) == 4 and all("k_select_negatives" in k for k in res), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 128, (name, r)
