"""Every form of the LayerNorm row kernels (csrc/layernorm.hip) through the C ABI, one form per test: the operand-plane entry
points of the f32 engine, the keyed-dropout backward, the embedding forward with dropout and the stream correction byte, the
embedding backwards with dropout, and the ordered (SIMX_DETERMINISTIC=1) column / table gradients of the four backward launchers.

Outputs that the kernels compute row by row (y, dz, the masked dz, the plane pairs) are compared BIT for bit with the plain
entry point on the same input and with the two roundings hi = rnd16(v), lo = rnd16(v - hi) done in torch; sums that go through
f32 atomics are compared with the float64 oracle at the tolerances of tests/test_kernels_gpu.py.  T = 37 rows: not a multiple
of the 4 waves of a workgroup, three workgroups in the forward, several rows per wave in the backward's grid-strided walk;
H = 64 / 260 / 768 / 1024: one vector per lane with 16 live lanes, three with a ragged last one, three full, four.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bert as obert
from oracle import planes as oplanes
from tests.test_kernels_gpu import TOL, L, assert_close, back, code, rnd, rounded, tdt, to_dev

pytestmark = pytest.mark.gpu

T = 37
HS = [64, 260, 768, 1024]
H16 = [True, "f16"]
EPS = 1e-12
P, SEED, STREAM = 0.1, 4321, 5
F16, BF16 = torch.float16, torch.bfloat16
# ragged sequence lengths (and position offsets) of test_embed_ln_bwd_position_major; the wider rows ride on the first set
EMBED_BWD = [([128, 1, 17, 33, 128, 100, 7], 0, 64), ([40] * 70, 2, 64), ([5, 300, 64], 0, 64),
             ([128, 1, 17, 33, 128, 100, 7], 0, 260), ([128, 1, 17, 33, 128, 100, 7], 0, 768), ([128, 1, 17, 33, 128, 100, 7], 0, 1024)]


def f64(a):
    return a.astype(np.float64)


@functools.lru_cache(maxsize=None)
def ln_case(H):
    """-> z, dy, gamma, beta (f32 arrays, shared by the tests of one H: nobody writes to them)"""
    return rnd((T, H), 1, 2.0) + 0.3, rnd((T, H), 2), 1.0 + rnd((H,), 3, 0.1), rnd((H,), 4, 0.1)


@functools.lru_cache(maxsize=None)
def ln_ref(H, fmt):
    """float64 oracle on the rounded inputs -> y, dx, dgamma, dbeta"""
    z, dy, g, b = ln_case(H)
    y, cache = obert._ln_fwd(rounded(z, fmt), f64(g), f64(b), EPS)
    dx, dg, db = obert._ln_bwd(rounded(dy, fmt), cache, f64(g))
    return y, dx, dg, db


def mult(rows, H, p=P):
    """[len(rows), H] f32 dropout multipliers of the (SEED, STREAM) mask"""
    return obert.drop_multipliers(p, SEED, STREAM, rows, np.arange(H)).astype(np.float32)


def split(v, t):
    """plane pair of an f32 tensor (oracle/planes.py), on the tensor's device"""
    hi, lo = oplanes.split16(v, t)
    return hi.to(v.device), lo.to(v.device)


def assert_planes(planes, v, t, what):
    hi, lo = split(v, t)
    assert torch.equal(planes[0].view(t), hi), what + ": hi plane"
    assert torch.equal(planes[1].view(t), lo), what + ": lo plane"


def new_planes(rows, H, dev):
    return torch.full((2, rows, H), -1, device=dev, dtype=torch.int16)


# ------------------------------------------------------------------------------------------ operand planes (f32 engine)
@pytest.mark.parametrize("H", HS)
def test_ln_fwd_planes(dev, H):
    lib = L()
    z, _, g, b = ln_case(H)
    z_d, g_d, b_d = to_dev(z, dev), to_dev(g, dev), to_dev(b, dev)
    y0, y1, pl = torch.empty_like(z_d), torch.empty_like(z_d), new_planes(T, H, dev)
    lib.call("simx_ln_fwd", lib.stream_ptr(), 0, T, H, lib.ptr(z_d), lib.ptr(g_d), lib.ptr(b_d), EPS, lib.ptr(y0))
    lib.call("simx_ln_fwd_planes", lib.stream_ptr(), T, H, lib.ptr(z_d), lib.ptr(g_d), lib.ptr(b_d), EPS, lib.ptr(y1), lib.ptr(pl), T * H)
    torch.cuda.synchronize()
    assert_close(back(y0), ln_ref(H, False)[0], what="ln_fwd", **TOL[False])
    assert torch.equal(y1, y0)
    assert_planes(pl, y1, F16, "ln_fwd_planes")


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("H", HS)
def test_ln_bwd_planes(dev, H, p):
    lib = L()
    z, dy, g, _ = ln_case(H)
    z_d, dy_d, g_d = to_dev(z, dev), to_dev(dy, dev), to_dev(g, dev)
    drop = lib.Dropout(p, SEED, STREAM)
    m = mult(np.arange(T), H, p)
    dz0, dzm0, dz1 = torch.empty_like(z_d), torch.full_like(z_d, float("nan")), torch.empty_like(z_d)
    pl = new_planes(T, H, dev)
    s0, s1 = torch.zeros(3, H, device=dev), torch.zeros(3, H, device=dev)
    lib.call("simx_ln_bwd_ex", lib.stream_ptr(), 0, T, H, lib.ptr(z_d), lib.ptr(g_d), EPS, lib.ptr(dy_d), lib.ptr(dz0), lib.ptr(dzm0),
             lib.ptr(s0[0]), lib.ptr(s0[1]), lib.ptr(s0[2]), C.byref(drop))
    lib.call("simx_ln_bwd_planes", lib.stream_ptr(), T, H, lib.ptr(z_d), lib.ptr(g_d), EPS, lib.ptr(dy_d), lib.ptr(dz1), lib.ptr(pl), T * H,
             lib.ptr(s1[0]), lib.ptr(s1[1]), lib.ptr(s1[2]), C.byref(drop))
    torch.cuda.synchronize()
    _, dx, dg, db = ln_ref(H, False)
    assert_close(back(dz0), dx, what="ln_bwd_ex dz", **TOL[False])
    assert torch.equal(dz1, dz0)
    masked = dz1 * to_dev(m, dev)                         # one f32 multiply per element, as in the kernel
    if p:
        assert torch.equal(dzm0, masked)
        assert (masked[to_dev(m, dev) == 0] == 0).all()
    assert_planes(pl, masked, BF16, "ln_bwd_planes")
    for s, who in ((s0, "ln_bwd_ex"), (s1, "ln_bwd_planes")):
        assert_close(back(s[0]), dg, rtol=1e-4, atol=1e-3, what=who + " dgamma")
        assert_close(back(s[1]), db, rtol=1e-4, atol=1e-3, what=who + " dbeta")
        assert_close(back(s[2]), (dx * m).sum(0), rtol=1e-4, atol=2e-3, what=who + " dbias")


# ------------------------------------------------------------------------------------------ keyed dropout (gathered rows)
@pytest.mark.parametrize("fmt", [False, True, "f16"])
@pytest.mark.parametrize("H", HS)
def test_ln_bwd_keyed(dev, H, fmt):
    lib = L()
    z, dy, g, _ = ln_case(H)
    keys = np.random.RandomState(9).permutation(5 * T)[:T].astype(np.int32)       # rows gathered out of a larger tensor
    z_d, dy_d, g_d, keys_d = to_dev(z, dev, fmt), to_dev(dy, dev, fmt), to_dev(g, dev), to_dev(keys, dev)
    drop = lib.Dropout(P, SEED, STREAM)
    dz, dzm = torch.empty_like(z_d), torch.full_like(z_d, float("nan"))
    s = torch.zeros(3, H, device=dev)
    lib.call("simx_ln_bwd_keyed", lib.stream_ptr(), code(fmt), T, H, lib.ptr(z_d), lib.ptr(g_d), EPS, lib.ptr(dy_d), lib.ptr(dz), lib.ptr(dzm),
             lib.ptr(s[0]), lib.ptr(s[1]), lib.ptr(s[2]), C.byref(drop), lib.ptr(keys_d))
    torch.cuda.synchronize()
    _, dx, dg, db = ln_ref(H, fmt)
    m32 = mult(keys, H)
    m = f64(m32)
    assert 0.05 < (m == 0).mean() < 0.15 and not np.array_equal(m, f64(mult(np.arange(T), H)))
    assert_close(back(dz), dx, what="ln_bwd_keyed dz", **TOL[fmt])
    assert_close(back(dzm), dx * m, what="ln_bwd_keyed dz_masked", **TOL[fmt])
    assert (back(dzm)[m == 0] == 0).all() and (back(dzm)[m != 0] != 0).mean() > 0.99
    if not fmt:
        assert torch.equal(dzm, dz * to_dev(m32, dev))     # f32: the masked copy is dz x multiplier, one f32 multiply per element
    else:
        # 16-bit: dz and the masked copy are each ONE rounding (relative error u) of the f32 dz and dz x multiplier, so per element
        # |dz_masked - dz x multiplier| <= 2 u |dz x multiplier| (2.1: the bound is taken at the rounded dz); 1e-7 covers fp16 subnormals
        u = 2.0 ** -8 if fmt is True else 2.0 ** -11
        assert (np.abs(back(dzm) - back(dz) * m) <= 2.1 * u * np.abs(back(dz) * m) + 1e-7).all()
    assert_close(back(s[0]), dg, rtol=1e-4, atol=1e-3, what="dgamma")
    assert_close(back(s[1]), db, rtol=1e-4, atol=1e-3, what="dbeta")
    assert_close(back(s[2]), (dx * m).sum(0), rtol=1e-4, atol=2e-3, what="dbias")


# ------------------------------------------------------------------------------------------ embedding forward
@functools.lru_cache(maxsize=None)
def embed_case(H, lens=None, off=0):
    """ids / positions / tables of an embedding test.  lens None: T random rows; else the packed ragged batch of
    test_embed_ln_bwd_position_major ([CLS] id collisions, in-sequence positions + off)."""
    V = 300
    if lens is None:
        rs = np.random.RandomState(0)
        n, Pn = T, 40
        ids = rs.randint(0, V, size=n).astype(np.int32)
        ids[:9] = 7
        pos = rs.randint(0, Pn, size=n).astype(np.int32)
        cu = None
    else:
        rs = np.random.RandomState(len(lens))
        n, Pn = sum(lens), max(lens) + off
        ids = rs.randint(0, V, size=n).astype(np.int32)
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ids[cu[:-1]] = 7                                  # [CLS] collisions
        pos = np.concatenate([np.arange(k) + off for k in lens]).astype(np.int32)
    word, posw, typew = rnd((V, H), 1), rnd((Pn, H), 2), rnd((2, H), 3)
    g, b = 1.0 + rnd((H,), 4, 0.1), rnd((H,), 5, 0.1)
    dy = rnd((n, H), 6)
    e = f64(word[ids] + posw[pos] + typew[0][None])
    y, cache = obert._ln_fwd(e, f64(g), f64(b), EPS)
    return dict(n=n, V=V, P=Pn, ids=ids, pos=pos, cu=cu, word=word, posw=posw, typew=typew, g=g, b=b, dy=dy, y=y, cache=cache)


@pytest.mark.parametrize("with_lo", [False, True])
@pytest.mark.parametrize("fmt", H16)
@pytest.mark.parametrize("H", HS)
def test_embed_ln_fwd_lo(dev, H, fmt, with_lo):
    lib = L()
    c = embed_case(H)
    d = lambda k: to_dev(c[k], dev)
    keep = [d("ids"), d("pos"), d("word"), d("posw"), d("typew"), d("g"), d("b")]
    drop = lib.Dropout(P, SEED, STREAM)
    out = torch.empty(T, H, device=dev, dtype=tdt(fmt))
    lo = torch.zeros(T, H, device=dev, dtype=torch.uint8) if with_lo else None
    lib.call("simx_embed_ln_fwd_lo", lib.stream_ptr(), code(fmt), T, H, *[lib.ptr(t) for t in keep], EPS, lib.ptr(out), lib.ptr(lo), C.byref(drop))
    m = f64(mult(np.arange(T), H))
    ref = c["y"] * m
    if not with_lo:
        torch.cuda.synchronize()
        assert_close(back(out), ref, what="embed_ln_fwd_lo", **TOL[fmt])
        assert (back(out)[m == 0] == 0).all()
        return
    dec = torch.empty(T, H, device=dev)
    lib.call("simx_stream_rows", lib.stream_ptr(), code(fmt), T, H, None, lib.ptr(out), lib.ptr(lo), None, None, lib.ptr(dec))
    torch.cuda.synchronize()
    assert int(lo.min()) >= 1
    eps2 = 2.0 ** -18 if fmt == "f16" else 2.0 ** -15      # the decoded stream of test_fp16_gpu.py::test_ln_residual_stream
    err = np.abs(back(dec) - ref).max()
    assert err <= eps2 * max(1.0, np.abs(ref).max()) + 1e-6, err
    assert (back(dec)[m == 0] == 0).all()


@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("H", HS)
def test_embed_ln_fwd_planes(dev, H, p):
    lib = L()
    c = embed_case(H)
    d = lambda k: to_dev(c[k], dev)
    keep = [d("ids"), d("pos"), d("word"), d("posw"), d("typew"), d("g"), d("b")]
    drop = lib.Dropout(p, SEED, STREAM)
    o0, o1, pl = torch.empty(T, H, device=dev), torch.empty(T, H, device=dev), new_planes(T, H, dev)
    lib.call("simx_embed_ln_fwd_ex", lib.stream_ptr(), 0, T, H, *[lib.ptr(t) for t in keep], EPS, lib.ptr(o0), C.byref(drop))
    lib.call("simx_embed_ln_fwd_planes", lib.stream_ptr(), T, H, *[lib.ptr(t) for t in keep], EPS, lib.ptr(o1), lib.ptr(pl), T * H, C.byref(drop))
    if not p:                                              # the issue's reference: simx_embed_ln_fwd itself
        o2 = torch.empty(T, H, device=dev)
        lib.call("simx_embed_ln_fwd", lib.stream_ptr(), 0, T, H, *[lib.ptr(t) for t in keep], EPS, lib.ptr(o2))
        torch.cuda.synchronize()
        assert torch.equal(o2, o0)
    torch.cuda.synchronize()
    assert_close(back(o0), c["y"] * f64(mult(np.arange(T), H, p)), what="embed_ln_fwd", **TOL[False])
    assert torch.equal(o1, o0)
    assert_planes(pl, o1, F16, "embed_ln_fwd_planes")


# ------------------------------------------------------------------------------------------ embedding backward with dropout
def embed_bwd_ref(c, fmt, p):
    """float64 oracle fed dy x multiplier -> dword, dpos, dtype0, dgamma, dbeta"""
    H = c["word"].shape[1]
    m = f64(mult(np.arange(c["n"]), H, p))
    de, dg, db = obert._ln_bwd(rounded(c["dy"], fmt) * m, c["cache"], f64(c["g"]))
    rw, rp = np.zeros((c["V"], H)), np.zeros((c["P"], H))
    np.add.at(rw, c["ids"], de)
    np.add.at(rp, c["pos"], de)
    return rw, rp, de.sum(0), dg, db


def embed_bwd_run(lib, dev, c, fmt, p, which, gs=None):
    """one embedding backward (which: "ex" row-major / "seq" position-major) -> [dword, dpos, dtype, dgamma, dbeta] tensors"""
    H, n = c["word"].shape[1], c["n"]
    d = lambda k: to_dev(c[k], dev)
    dy = to_dev(c["dy"] * (gs[0] if gs else 1.0), dev, fmt)       # (a power-of-two loss scale: exact in every format)
    dgs = torch.tensor(gs, device=dev) if gs else None
    drop = lib.Dropout(p, SEED, STREAM)
    tabs = [d("ids"), d("pos"), d("word"), d("posw"), d("typew"), d("g")]
    outs = [torch.zeros(c["V"], H, device=dev), torch.zeros(c["P"], H, device=dev), torch.zeros(2, H, device=dev),
            torch.zeros(H, device=dev), torch.zeros(H, device=dev)]
    if which == "ex":
        assert gs is None
        lib.call("simx_embed_ln_bwd_ex", lib.stream_ptr(), code(fmt), n, H, *[lib.ptr(t) for t in tabs], EPS, lib.ptr(dy),
                 *[lib.ptr(t) for t in outs], C.byref(drop))
    else:
        cu = d("cu")
        lens = np.diff(c["cu"])
        lib.call("simx_embed_ln_bwd_seq_gs", lib.stream_ptr(), code(fmt), len(lens), int(lens.max()), n, H, lib.ptr(cu),
                 *[lib.ptr(t) for t in tabs], EPS, lib.ptr(dy), *[lib.ptr(t) for t in outs], C.byref(drop), lib.ptr(dgs))
    torch.cuda.synchronize()
    return outs


def embed_bwd_check(outs, ref, which):
    # test_embed_ln (row-major) / test_embed_ln_bwd_position_major (position-major), without dropout
    a_tab, a_col = (1e-4, 1e-3) if which == "ex" else (2e-4, 2e-3)
    gw, gp, gt, gg, gb = (back(t) for t in outs)
    rw, rp, rt, dg, db = ref
    assert_close(gw, rw, rtol=1e-4, atol=a_tab, what=which + " dword")
    assert_close(gp, rp, rtol=1e-4, atol=a_tab, what=which + " dpos")
    assert_close(gt[0], rt, rtol=1e-4, atol=a_col, what=which + " dtype0")
    assert np.abs(gt[1]).max() == 0.0
    assert_close(gg, dg, rtol=1e-4, atol=a_col, what=which + " dgamma")
    assert_close(gb, db, rtol=1e-4, atol=a_col, what=which + " dbeta")


@pytest.mark.parametrize("fmt", [False, True, "f16"])
@pytest.mark.parametrize("lens,off,H", EMBED_BWD)
def test_embed_ln_bwd_dropout(dev, fmt, lens, off, H):
    lib = L()
    c = embed_case(H, tuple(lens), off)
    ref = embed_bwd_ref(c, fmt, P)
    assert np.abs(ref[0] - embed_bwd_ref(c, fmt, 0.0)[0]).max() > 0.05      # the mask matters at these tolerances
    for which in ("ex", "seq"):
        embed_bwd_check(embed_bwd_run(lib, dev, c, fmt, P, which), ref, which)


# ------------------------------------------------------------------------------------------ deterministic mode
def _det_worker():
    """One process (SIMX_DETERMINISTIC is read once per process): the four backward launchers twice each on the shapes above;
    every output of the two runs is torch.equal, and agrees with the oracle at the tolerances of the atomic mode."""
    lib = L()
    assert lib.load().simx_deterministic() == 1
    dev = torch.device("cuda:0")
    drop = lib.Dropout(P, SEED, STREAM)
    m = {H: mult(np.arange(T), H) for H in HS}

    def twice(fn, what):
        a, b = fn(), fn()
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), "%s: output %d differs between two runs" % (what, i)
        return a

    for H in HS:
        z, dy, g, _ = ln_case(H)
        g_d = to_dev(g, dev)
        # simx_ln_bwd_res, fp16 residual stream with the correction byte, dropout: z = d + r_hi + r_lo
        rq = np.random.RandomState(7).randint(1, 256, size=(T, H)).astype(np.uint8)
        dd, rh, rl, dy16 = to_dev(z * 0.5, dev, "f16"), to_dev(z * 0.5 + 0.1, dev, "f16"), to_dev(rq, dev), to_dev(dy, dev, "f16")
        r32 = torch.empty(T, H, device=dev)
        lib.call("simx_stream_rows", lib.stream_ptr(), 2, T, H, None, lib.ptr(rh), lib.ptr(rl), None, None, lib.ptr(r32))

        def res():
            dz, dzm, s = torch.empty_like(dd), torch.empty_like(dd), torch.zeros(3, H, device=dev)
            lib.call("simx_ln_bwd_res", lib.stream_ptr(), 2, T, H, lib.ptr(dd), lib.ptr(rh), lib.ptr(rl), lib.ptr(g_d), EPS, lib.ptr(dy16),
                     lib.ptr(dz), lib.ptr(dzm), lib.ptr(s[0]), lib.ptr(s[1]), lib.ptr(s[2]), C.byref(drop), None, None)
            torch.cuda.synchronize()
            return dz, dzm, s
        dz, dzm, s = twice(res, "ln_bwd_res H=%d" % H)
        _, cache = obert._ln_fwd(back(dd) + back(r32), f64(g), np.zeros(H), EPS)
        dx, dgr, dbr = obert._ln_bwd(back(dy16), cache, f64(g))
        assert_close(back(dz), dx, what="det ln_bwd_res dz", **TOL["f16"])
        assert_close(back(dzm), dx * m[H], what="det ln_bwd_res dz_masked", **TOL["f16"])
        assert_close(back(s[0]), dgr, rtol=1e-4, atol=1e-3, what="det ln_bwd_res dgamma")
        assert_close(back(s[1]), dbr, rtol=1e-4, atol=1e-3, what="det ln_bwd_res dbeta")
        assert_close(back(s[2]), (dx * m[H]).sum(0), rtol=1e-4, atol=2e-3, what="det ln_bwd_res dbias")

        # simx_ln_bwd_planes, f32, dropout
        z32, dy32 = to_dev(z, dev), to_dev(dy, dev)

        def planes():
            dz, pl, s = torch.empty_like(z32), new_planes(T, H, dev), torch.zeros(3, H, device=dev)
            lib.call("simx_ln_bwd_planes", lib.stream_ptr(), T, H, lib.ptr(z32), lib.ptr(g_d), EPS, lib.ptr(dy32), lib.ptr(dz), lib.ptr(pl), T * H,
                     lib.ptr(s[0]), lib.ptr(s[1]), lib.ptr(s[2]), C.byref(drop))
            torch.cuda.synchronize()
            return dz, pl, s
        dz, pl, s = twice(planes, "ln_bwd_planes H=%d" % H)
        _, dx, dgr, dbr = ln_ref(H, False)
        assert_close(back(dz), dx, what="det ln_bwd_planes dz", **TOL[False])
        assert_planes(pl, dz * to_dev(m[H], dev), BF16, "det ln_bwd_planes")
        assert_close(back(s[0]), dgr, rtol=1e-4, atol=1e-3, what="det ln_bwd_planes dgamma")
        assert_close(back(s[1]), dbr, rtol=1e-4, atol=1e-3, what="det ln_bwd_planes dbeta")
        assert_close(back(s[2]), (dx * m[H]).sum(0), rtol=1e-4, atol=2e-3, what="det ln_bwd_planes dbias")

    # the embedding backwards: f32 and fp16 rows, dropout; the position-major one with a loss scale of 4
    for (lens, off, H), fmt in zip(EMBED_BWD, [False, "f16", True, "f16", False, True]):
        c = embed_case(H, tuple(lens), off)
        ref = embed_bwd_ref(c, fmt, P)
        embed_bwd_check(twice(lambda: embed_bwd_run(lib, dev, c, fmt, P, "ex"), "embed_ln_bwd_ex H=%d" % H), ref, "ex")
        embed_bwd_check(twice(lambda: embed_bwd_run(lib, dev, c, fmt, P, "seq", gs=[4.0, 0.25]), "embed_ln_bwd_seq_gs H=%d" % H), ref, "seq")
    print("det worker OK")


def test_deterministic_backward_launchers(dev):
    """SIMX_DETERMINISTIC=1 in one child process: simx_ln_bwd_res, simx_ln_bwd_planes, simx_embed_ln_bwd_ex and
    simx_embed_ln_bwd_seq_gs give the same bits twice and agree with the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SIMX_DETERMINISTIC="1")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    prog = "import sys; sys.path.insert(0, %r); from tests.test_ln_forms_gpu import _det_worker; _det_worker()" % root
    r = subprocess.run([sys.executable, "-c", prog], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "det worker OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
