"""Host side of the fold-in of unseen users (include/dcue.h dcue_user_foldin, added under ABI 17), no
GPU needed: header, binding and library agree on the new symbols and the config struct, every
bad-argument return (validated on the host before the first device call), the workspace formula, the
torch reference's self-checks (foldin_reference.py) and the compiled kernels' scratch use."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import foldin_reference as R
from conftest import ROOT
from kernel_resources import HIPCC, kernel_resources

HEADER = os.path.join(ROOT, "include", "dcue.h")
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
NEW = ("dcue_foldin_workspace_bytes", "dcue_user_foldin", "dcue_foldin_negatives")


# ------------------------------------------------------------------------------- ABI
def test_symbols_in_header_binding_and_library():
    from dcrecommend import _native as nat
    src = open(HEADER).read()
    declared = set(re.findall(r"^int\s*(dcue_\w+)\s*\(", src, flags=re.M))
    lib = nat.lib()
    for name in NEW:
        assert name in declared, name
        assert name in nat._SIGS, name
        assert hasattr(lib, name), name
    assert "added under ABI 17" in src
    assert int(re.search(r"#define DCUE_ABI_VERSION (\d+)", src).group(1)) == 17
    assert nat.ABI_VERSION == 17 and lib.dcue_abi_version() == 17


def test_foldin_config_matches_header(tmp_path):
    from dcrecommend import _native as nat
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcue.h"', "int main(void) {",
           'printf("dcue_foldin_config %zu\\n", sizeof(dcue_foldin_config));']
    for fname, _ in nat.FoldinConfig._fields_:
        src.append('printf("%s %%zu\\n", offsetof(dcue_foldin_config, %s));' % (fname, fname))
    src.append("return 0; }")
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"),
                           "-o", str(tmp_path / "probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    assert int(got["dcue_foldin_config"]) == ctypes.sizeof(nat.FoldinConfig)
    for fname, _ in nat.FoldinConfig._fields_:
        assert int(got[fname]) == getattr(nat.FoldinConfig, fname).offset, fname
    hdr = open(HEADER).read()
    for lim, text in ((nat.FOLDIN_MAX_STEPS, "0..4096"), (nat.FOLDIN_MAX_NEG, "1..256"), (nat.FOLDIN_MAX_POS, "1..1024")):
        assert text in hdr and text.endswith(str(lim))


# ------------------------------------------------------------------------------- bad arguments
def _dims(E=300, d=100, H=128):
    from dcrecommend import _native as nat
    return nat.Dims(H, d, E, 0, 10, 0, 0, 0, 0)


def _cfg(**over):
    from dcrecommend import _native as nat
    a = dict(steps=30, n_neg=20, max_pos=64, margin=0.2, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8,
             weight_decay=0.0, seed=0)
    a.update(over)
    return nat.FoldinConfig(*[a[n] for n, _ in nat.FoldinConfig._fields_])


def _call(config=None, dims=None, **over):
    """dcue_user_foldin with device arguments that are never dereferenced: every case returns before
    a device call."""
    from dcrecommend import _native as nat
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    m = nat.Model()
    m.dims = dims if dims is not None else _dims()
    m.params = m.bn_stats = m.bn_batches = m.wpack = p.value
    cfg = config if config is not None else _cfg()
    a = dict(m=ctypes.byref(m), cand_feat=p, n_cand=1000, cand_mask=p, hist_ptr=p, hist_idx=p, n_users=4, row0=0,
             cfg=ctypes.byref(cfg), emb=p, ws=p, ws_bytes=0, out_feat=p, out_loss=p, out_grad=p, out_flags=p,
             stream=None)
    a.update(over)
    order = ("m", "cand_feat", "n_cand", "cand_mask", "hist_ptr", "hist_idx", "n_users", "row0", "cfg", "emb", "ws",
             "ws_bytes", "out_feat", "out_loss", "out_grad", "out_flags", "stream")
    return nat.lib().dcue_user_foldin(*[a[n] for n in order])


@pytest.mark.parametrize("name", ["m", "cand_feat", "hist_ptr", "hist_idx", "cfg", "emb", "ws", "out_feat",
                                  "out_flags"])
def test_foldin_null_pointer_is_invalid(name):
    assert _call(**{name: None}) == INVALID


@pytest.mark.parametrize("over", [dict(n_neg=0), dict(n_neg=257), dict(max_pos=0), dict(max_pos=1025),
                                  dict(steps=-1), dict(steps=4097)])
def test_foldin_config_out_of_range_is_invalid(over):
    assert _call(config=_cfg(**over)) == INVALID


def test_foldin_other_argument_errors():
    assert _call(n_cand=0) == INVALID
    assert _call(n_cand=-5) == INVALID
    assert _call(dims=_dims(d=257)) == UNSUPPORTED
    assert _call(dims=_dims(E=1025)) == UNSUPPORTED
    assert _call(dims=_dims(E=1024, d=256), n_users=0) == OK
    # valid arguments, a workspace of 0 bytes: refused on the host
    assert _call() == WORKSPACE
    assert _call(cand_mask=None, out_loss=None, out_grad=None) == WORKSPACE
    assert _call(config=_cfg(steps=0, n_neg=256, max_pos=1024)) == WORKSPACE
    assert _call(n_users=0) == OK  # nothing to do


def test_negatives_argument_errors():
    from dcrecommend import _native as nat
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cfg = _cfg()
    f = nat.lib().dcue_foldin_negatives
    assert f(1000, p, p, p, 0, 0, ctypes.byref(cfg), 0, p, None) == OK  # no rows
    assert f(1000, p, None, p, 4, 0, ctypes.byref(cfg), 0, p, None) == INVALID
    assert f(1000, p, p, p, 4, 0, ctypes.byref(cfg), 0, None, None) == INVALID
    assert f(1000, p, p, p, 4, 0, None, 0, p, None) == INVALID
    assert f(0, p, p, p, 4, 0, ctypes.byref(cfg), 0, p, None) == INVALID
    assert f(1000, p, p, p, 4, 0, ctypes.byref(cfg), -1, p, None) == INVALID
    assert f(1000, p, p, p, 4, 0, ctypes.byref(_cfg(n_neg=0)), 0, p, None) == INVALID


# ------------------------------------------------------------------------------- workspace
def _ws(dims, n_cand, n_users, max_pos, n_neg):
    from dcrecommend import _native as nat
    n = ctypes.c_size_t(0)
    st = nat.lib().dcue_foldin_workspace_bytes(ctypes.byref(dims) if dims is not None else None, n_cand, n_users,
                                               max_pos, n_neg, ctypes.byref(n))
    return st, n.value


@pytest.mark.parametrize("E,d", [(40, 32), (300, 100), (300, 128), (512, 128), (1024, 256)])
def test_workspace_bytes(E, d):
    dims = _dims(E, d)
    st, base = _ws(dims, 200000, 4096, 64, 20)
    assert st == OK and base >= 200000 * ((d + 15) // 16 * 16) * 4, "the normalised candidates live in the workspace"
    sizes = [_ws(dims, 200000, n, 64, 20)[1] for n in (0, 1, 16, 17, 1000, 4096, 20000)]
    assert sizes == sorted(sizes), ("n_users", sizes)
    sizes = [_ws(dims, 200000, 4096, p, 20)[1] for p in (1, 16, 64, 1024)]
    assert sizes == sorted(sizes), ("max_pos", sizes)
    sizes = [_ws(dims, 200000, 4096, 64, n)[1] for n in (1, 5, 20, 256)]
    assert sizes == sorted(sizes), ("n_neg", sizes)
    # nothing of size n_users x n_cand, no gathered factor rows [n_users][max_pos (1 + n_neg)][d]
    assert base < 4096 * 200000 * 4 // 10
    assert base - 200000 * ((d + 15) // 16 * 16) * 4 < 4096 * 64 * 21 * d * 4 // 10


def test_workspace_config2_bound():
    """BASELINE config 2 (200,000 candidates, d = 128, E = 300, 4,096 new users): below one tenth of
    n_users x n_cand x 4 bytes."""
    st, n = _ws(_dims(300, 128), 200000, 4096, 64, 20)
    assert st == OK and n < 4096 * 200000 * 4 // 10


def test_workspace_bytes_errors():
    from dcrecommend import _native as nat
    assert _ws(None, 1000, 4, 64, 20)[0] == INVALID
    assert nat.lib().dcue_foldin_workspace_bytes(ctypes.byref(_dims()), 1000, 4, 64, 20, None) == INVALID
    assert _ws(_dims(), 0, 4, 64, 20)[0] == INVALID
    assert _ws(_dims(), 1000, -1, 64, 20)[0] == INVALID
    assert _ws(_dims(), 1000, 4, 0, 20)[0] == INVALID
    assert _ws(_dims(), 1000, 4, 1025, 20)[0] == INVALID
    assert _ws(_dims(), 1000, 4, 64, 0)[0] == INVALID
    assert _ws(_dims(), 1000, 4, 64, 257)[0] == INVALID
    assert _ws(_dims(d=257), 1000, 4, 64, 20)[0] == UNSUPPORTED
    assert _ws(_dims(E=1025), 1000, 4, 64, 20)[0] == UNSUPPORTED


# ------------------------------------------------------------------------------- the reference
def test_sampler_vectors():
    """First-attempt draws (t = 7, i = 3, j = 0..3, 1,000 candidates, nothing rejected) and row keys
    for two seeds and two rows, computed independently (a C restatement of the header's formulas)."""
    want = {(0, 0): (16294208416658607535, [35, 286, 201, 677]),
            (0, 1000): (3240954710329600481, [605, 625, 99, 777]),
            (12345678901234567, 0): (13463060612230490842, [996, 273, 66, 743]),
            (12345678901234567, 1000): (10998324083615161681, [602, 181, 377, 84])}
    for (seed, r), (z0, draws) in want.items():
        assert R.row_key(seed, r) == z0
        assert [R.negative(z0, 7, 3, j, 1000, None, []) for j in range(4)] == draws
    # a rejected first attempt moves on to the second: the draw changes, and only for that slot
    mask = np.ones(1000, np.uint8)
    mask[35] = 0
    z0 = want[(0, 0)][0]
    got = [R.negative(z0, 7, 3, j, 1000, mask, []) for j in range(4)]
    assert got[0] != 35 and got[0] >= 0 and got[1:] == [286, 201, 677]
    assert R.negative(z0, 7, 3, 1, 1000, None, [286]) not in (286, -1)
    # batching: a row's draws depend on its global index alone
    a = R.negatives(5, 1000, 2, [3, 9], 4, 3, 1000, None)
    assert a.shape == (4, 3) and np.all(a[:2] >= 0) and np.all(a[2:] == -1)
    assert not np.array_equal(a, R.negatives(5, 1001, 2, [3, 9], 4, 3, 1000, None))


def test_sampler_rejected_slots():
    """A history that covers all but two eligible candidates: every accepted draw is one of the two,
    and with 8 attempts at 2 in 50 most slots are dropped."""
    n_cand = 50
    mask = np.ones(n_cand, np.uint8)
    mask[[4, 30]] = 0
    keep = [11, 41]
    hist = [c for c in range(n_cand) if mask[c] and c not in keep]
    neg = R.negatives(3, 0, 0, hist, 16, 20, n_cand, mask)
    assert set(np.unique(neg)) <= {-1, 11, 41}
    assert (neg == -1).sum() > neg.size // 2 and (neg >= 0).any()
    W = (np.eye(8, dtype=np.float32), np.zeros(8, np.float32), np.eye(8, dtype=np.float32), np.zeros(8, np.float32))
    rs = np.random.RandomState(0)
    cand, init = rs.randn(n_cand, 8), rs.randn(2, 8)
    out = R.fold_in(W, cand, mask, [hist, []], init, 2, 20, 16, 0.2, 0.05, seed=3)
    assert out["flags"].tolist() == [R.DROPPED, R.EMPTY]
    assert np.all(out["loss"][1] == 0) and np.array_equal(out["emb"][1], init[1])  # an empty history: untouched
    assert not np.array_equal(out["emb"][0], init[0])
    assert np.isfinite(out["loss"]).all()


def test_rotating_window():
    hist = list(range(100, 110))
    assert R.positives(hist, 0, 4) == [100, 101, 102, 103]
    assert R.positives(hist, 1, 4) == [104, 105, 106, 107]
    assert R.positives(hist, 2, 4) == [108, 109, 100, 101]
    assert R.positives(hist, 5, 4) == [100, 101, 102, 103]  # 20 mod 10
    assert R.positives(hist, 0, 64) == hist  # the whole history when it fits,
    assert R.positives(hist, 3, 64) == hist[2:] + hist[:2]  # rotated by 3 * 64 mod 10
    assert R.positives(hist[:1], 9, 64) == hist[:1]


@pytest.mark.parametrize("case", R.ONE_STEP_CASES + R.TIER_CASES)
def test_one_step_cases_meet_the_condition(case):
    E, d, n_cand, n_neg, seed = case
    c = R.make_case(E, d, n_cand, R.ONE_STEP_LENS, seed)
    r64 = R.reference(c, torch.float64, n_neg=n_neg, **R.ONE_STEP_CFG)
    r32 = R.reference(c, torch.float32, n_neg=n_neg, **R.ONE_STEP_CFG)
    dl, dg = R.spread(r32, r64)
    print("one step %s: fp32-vs-fp64 spread loss %.3e, gradient %.3e of the row's largest |g|" % (case, dl, dg))
    assert r64["hinge"].size > 0 and not (np.abs(r64["hinge"]) < R.NEAR_TIE).any()
    assert dl < 1e-5 and dg < 1e-5 and np.isfinite(r64["loss"]).all()
    # (the 200-song history leaves 47 % of the draws acceptable: a few of its slots are dropped)
    assert not (r64["flags"] & (R.EMPTY | R.NONFINITE)).any()


@pytest.mark.parametrize("case", R.THIRTY_CASES)
def test_thirty_step_cases_meet_the_condition(case):
    E, d, n_cand, n_neg, seed = case
    c = R.make_case(E, d, n_cand, R.THIRTY_LENS, seed)
    r64 = R.reference(c, torch.float64, n_neg=n_neg, **R.THIRTY_CFG)
    r32 = R.reference(c, torch.float32, n_neg=n_neg, **R.THIRTY_CFG)
    dl = float(np.abs(r32["loss"][:, -1].astype(np.float64) - r64["loss"][:, -1]).max())
    print("thirty steps %s: fp32-vs-fp64 spread of the final loss %.3e, of the rows %.3e"
          % (case, dl, float(np.abs(r32["emb"] - r64["emb"]).max())))
    near = int((np.abs(r64["hinge"]) < R.NEAR_TIE).sum())
    assert near <= r64["hinge"].size // 1000, (near, r64["hinge"].size)
    assert np.all(r64["loss"][:, -1] < r64["loss"][:, 0]), "every user's loss falls"


# ------------------------------------------------------------------------------- compiled kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_foldin_kernels_use_no_scratch(tmp_path):
    res = kernel_resources("foldin.hip", tmp_path, ["-ffp-contract=off"])
    found = {k: v for k, v in res.items() if "k_foldin" in k}
    assert len([k for k in found if "k_foldin_negatives" in k]) == 1
    assert len([k for k in found if "k_foldinILi" in k]) == 3, sorted(found)  # the three residency tiers
    for k, v in found.items():
        assert v.get("ScratchSize", -1) == 0, (k, v)
