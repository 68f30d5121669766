"""oracle/attention.py::mha_ref -- the float64 attention reference with the stateless dropout mask -- checked without a GPU:
against torch.autograd, against the older _mha_ref, and, together with the bounds of tests/attention_cases.py, for what the GPU
file tests/test_attention_edges_gpu.py can and cannot see:
  * sensitivity: a reference with a misplaced mask column, a misplaced mask row or an unscaled backward mask leaves the bound of
    every format at every length list, so a kernel with that fault fails;
  * a float64 emulation of a 16-bit kernel's rounding points stays inside the ramped-key bound, so that bound is not below the
    format's own rounding (a CPU emulation, not a GPU measurement).
"""
import math

import numpy as np
import pytest
import torch

from oracle import bert as obert
from oracle.attention import drop_mults, mha_ref
from tests import attention_cases as ac
from tests.test_kernels_gpu import _mha_ref


def _autograd(qkv, lens, heads, d, dctx, drop):
    T, H = qkv.shape[0], heads * d
    x = torch.from_numpy(qkv).clone().requires_grad_(True)
    ctx, lse = torch.zeros(T, H, dtype=torch.float64), torch.zeros(heads, T, dtype=torch.float64)
    rows, t0 = [], 0
    for n in lens:
        cols = []
        for h in range(heads):
            q, k, v = (x[t0:t0 + n, w * H + h * d:w * H + (h + 1) * d] for w in range(3))
            s = q @ k.T / math.sqrt(d)
            mult = torch.from_numpy(np.asarray(drop_mults(drop, T, h, t0, n)[0], dtype=np.float64) * np.ones((n, n)))
            cols.append((torch.softmax(s, 1) * mult) @ v)
            lse[h, t0:t0 + n] = torch.logsumexp(s, 1).detach()
        rows.append(torch.cat(cols, 1))
        t0 += n
    ctx = torch.cat(rows, 0)
    (ctx * torch.from_numpy(dctx)).sum().backward()
    return ctx.detach().numpy(), lse.numpy(), x.grad.numpy()


@pytest.mark.parametrize("drop", [None, (0.1, ac.SEED, ac.STREAM), (0.5, 7, 3)])
@pytest.mark.parametrize("lens", [[250, 1, 17, 5, 200, 33], ac.LISTS["R2"]])
def test_mha_ref_matches_autograd(lens, drop):
    qkv, dctx = (a.astype(np.float64) for a in ac.inputs(lens))
    got = mha_ref(qkv, lens, ac.HEADS, ac.D, dctx, drop)
    want = _autograd(qkv, lens, ac.HEADS, ac.D, dctx, drop)
    for g, w, what in zip(got, want, ("ctx", "lse", "dqkv")):
        err = np.abs(g - w).max()
        print("%s %.2e" % (what, err))
        assert err <= 1e-12, (what, err)


@pytest.mark.parametrize("heads,d,lens", [(3, 64, ac.LISTS["R8"]), (4, 16, [5, 32, 17, 1]), (2, 96, [40, 7, 130, 1])])
def test_mha_ref_without_dropout_is_the_old_reference(heads, d, lens):
    qkv, dctx = (a.astype(np.float64) for a in ac.inputs(lens, heads, d))
    for g, w in zip(mha_ref(qkv, lens, heads, d, dctx), _mha_ref(qkv, lens, heads, d, dctx)):
        assert np.array_equal(g, w)
    c, l, q = mha_ref(qkv, lens, heads, d)
    c0, l0, q0 = _mha_ref(qkv, lens, heads, d)
    assert q is None and q0 is None and np.array_equal(c, c0) and np.array_equal(l, l0)


def test_mask_is_keyed_by_head_and_packed_token():
    """rows = head * T + packed token, cols = key inside the sequence: the mask of (sequence 1, head 2) is the hash at those keys"""
    lens, heads, d = [5, 9], 3, 8
    T = sum(lens)
    m, _ = drop_mults((0.25, ac.SEED, ac.STREAM), T, 2, 5, 9)
    want = obert.drop_multipliers(0.25, ac.SEED, ac.STREAM, 2 * T + 5 + np.arange(9), np.arange(9))
    assert np.array_equal(m, want) and set(np.unique(m)) == {0.0, float(np.float32(4.0) / np.float32(3.0))}
    qkv = ac.rnd((T, 3 * heads * d), 5).astype(np.float64)
    c, l, _ = mha_ref(qkv, lens, heads, d, None, (0.25, ac.SEED, ac.STREAM))
    c0, l0, _ = mha_ref(qkv, lens, heads, d)
    assert np.array_equal(l, l0) and not np.array_equal(c, c0)            # lse is the undropped row's


# ------------------------------------------------------------------------------------------ sensitivity of the bounds
def _shift_cols(drop, T, h, t0, n):
    """(a) the last 16 keys use column key col + 4"""
    p, seed, stream = drop
    cols = np.arange(n)
    cols[-16:] += 4
    m = obert.drop_multipliers(p, seed, stream, h * T + t0 + np.arange(n), cols)
    return m, m


def _shift_last_row(drop, T, h, t0, n):
    """(b) the last query row uses row key row + 1"""
    p, seed, stream = drop
    rows = h * T + t0 + np.arange(n)
    rows[-1] += 1
    m = obert.drop_multipliers(p, seed, stream, rows, np.arange(n))
    return m, m


def _unscaled_backward(drop, T, h, t0, n):
    """(c) backward multipliers of 1 instead of 256 / (256 - thr) on kept entries"""
    m, _ = drop_mults(drop, T, h, t0, n)
    return m, (m > 0).astype(np.float64)


@pytest.mark.parametrize("name", list(ac.LISTS))
def test_bounds_see_a_misplaced_or_unscaled_mask(name):
    lens, drop = ac.LISTS[name], (0.1, ac.SEED, ac.STREAM)
    k = ac.drop_k(0.1)
    assert k == 256.0 / 230.0
    raw = ac.inputs(lens)
    for fmt, kinds in (("f32", ("f32", "pair")), ("f16", ("f16",)), ("bf16", ("bf16",))):     # the inputs a kernel sees; its bounds
        qkv, dctx = (ac.rounded(a, fmt) for a in raw)
        ref = mha_ref(qkv, lens, ac.HEADS, ac.D, dctx, drop)
        for fault in (_shift_cols, _shift_last_row, _unscaled_backward):
            bad = mha_ref(qkv, lens, ac.HEADS, ac.D, dctx, drop, mults=fault)
            for kind in kinds:
                lim = ac.limits(kind, ref, lens, ac.HEADS, ac.D, k)
                out = [int((np.abs(b - r) > l).sum()) for b, r, l in zip(bad, ref, lim)]
                print("%-5s %-4s %-20s elements out of bound: ctx %d lse %d dqkv %d" % (name, kind, fault.__name__, *out))
                assert out[1] == 0                       # lse is the undropped row's: no mask fault moves it
                assert out[0] + out[2] >= 1, (name, kind, fault.__name__)
                if fault is _unscaled_backward:
                    assert out[0] == 0                   # a backward-only fault: the forward is the reference's


# ------------------------------------------------------------------------------------------ the ramped bound against 16-bit rounding
def _emulate16(qkv, lens, heads, d, dctx, fmt):
    """float64 attention with a 16-bit kernel's rounding points: P, dS and the outputs rounded to the format (the inputs already
    are), delta = rowsum(dO * O) from the rounded O."""
    rd = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ac.TORCH_DT[fmt]).to(torch.float64).numpy()
    T, H = qkv.shape[0], heads * d
    ctx, lse, dqkv = np.zeros((T, H)), np.zeros((heads, T)), np.zeros_like(qkv)
    t0 = 0
    for n in lens:
        for h in range(heads):
            q, k, v = (qkv[t0:t0 + n, w * H + h * d:w * H + (h + 1) * d] for w in range(3))
            do = dctx[t0:t0 + n, h * d:(h + 1) * d]
            s = q @ k.T / math.sqrt(d)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            p = e / e.sum(1, keepdims=True)
            lse[h, t0:t0 + n] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
            p16 = rd(p)
            o = rd(p16 @ v)
            ctx[t0:t0 + n, h * d:(h + 1) * d] = o
            delta = (do * o).sum(1, keepdims=True)
            ds = rd(p * (do @ v.T - delta) / math.sqrt(d))
            dqkv[t0:t0 + n, h * d:(h + 1) * d] = rd(ds @ k)
            dqkv[t0:t0 + n, H + h * d:H + (h + 1) * d] = rd(ds.T @ q)
            dqkv[t0:t0 + n, 2 * H + h * d:2 * H + (h + 1) * d] = rd(p16.T @ do)
        t0 += n
    return ctx, lse, dqkv


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name", ["R16", "LONG", "LONG2"])
def test_ramped_bound_is_not_below_16_bit_rounding(name, direction, fmt):
    lens = ac.LISTS[name]
    qkv, dctx = (ac.rounded(a, fmt) for a in ac.inputs(lens, ramp=direction))
    ref = mha_ref(qkv, lens, ac.HEADS, ac.D, dctx)
    lim = ac.limits(fmt, ref, lens, ac.HEADS, ac.D, ramp=True)
    emu = _emulate16(qkv, lens, ac.HEADS, ac.D, dctx, fmt)
    ratios = [ac.worst(g, r, l) for g, r, l in zip(emu, ref, lim)]
    print("%-5s %-4s %-4s err/bound: ctx %.2f lse %.2f dqkv %.2f" % (name, direction, fmt, *ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name", ["R16", "LONG", "LONG2"])
def test_ramped_ctx_bound_of_the_f32_unit_against_f32_rounding(name, direction):
    """Why the planes form of the f32 unit has 6e-6 instead of 3e-6 on ctx with ramped keys: the scores reach +-40 there, where
    one f32 ulp is 3.8e-6, and a kernel that holds its scores in f32 cannot do better than a plain float32 attention (NumPy: f32
    products, exponentials and sums, nothing else rounded), which sits at 0.7 - 1.1 of 3e-6 * max|ctx| here.  x3 keeps 3e-6."""
    lens, H = ac.LISTS[name], ac.HEADS * ac.D
    qkv, _ = ac.inputs(lens, ramp=direction)
    ref = mha_ref(qkv.astype(np.float64), lens, ac.HEADS, ac.D)
    ctx = np.zeros_like(ref[0])
    t0 = 0
    for n in lens:
        for h in range(ac.HEADS):
            q, k, v = (qkv[t0:t0 + n, w * H + h * ac.D:w * H + (h + 1) * ac.D] for w in range(3))
            s = (q @ k.T) * np.float32(1.0 / math.sqrt(ac.D))
            e = np.exp(s - s.max(1, keepdims=True))
            assert e.dtype == np.float32
            ctx[t0:t0 + n, h * ac.D:(h + 1) * ac.D] = (e @ v) / e.sum(1, keepdims=True)
        t0 += n
    x3 = ac.worst(ctx, ref[0], ac.limits("pair", ref, lens, ac.HEADS, ac.D, ramp=True)[0])
    pl = ac.worst(ctx, ref[0], ac.limits("planes", ref, lens, ac.HEADS, ac.D, ramp=True)[0])
    print("%-5s %-4s float32 attention, ctx err/bound: 3e-6 form %.2f, planes form %.2f" % (name, direction, x3, pl))
    assert 0.25 <= x3 and pl <= 1.0, (x3, pl)


def test_ramp_and_limits_helpers():
    lens = [5, 1, 3]
    H = ac.HEADS * ac.D
    plain, _ = ac.inputs(lens)
    up, _ = ac.inputs(lens, ramp="up")
    down, _ = ac.inputs(lens, ramp="down")
    f = np.array([0.25, 1.1875, 2.125, 3.0625, 4.0, 0.25, 0.25, 2.125, 4.0], dtype=np.float32)[:, None]
    g = np.array([4.0, 3.0625, 2.125, 1.1875, 0.25, 0.25, 4.0, 2.125, 0.25], dtype=np.float32)[:, None]
    assert np.array_equal(up[:, :H], plain[:, :H] * 2) and np.array_equal(up[:, 2 * H:], plain[:, 2 * H:])
    assert np.array_equal(up[:, H:2 * H], plain[:, H:2 * H] * f) and np.array_equal(down[:, H:2 * H], plain[:, H:2 * H] * g)
    # the block maximum of the unramped case, the 3 of the ramped bound
    lens = ac.LISTS["R16"]
    qkv, dctx = (a.astype(np.float64) for a in ac.inputs(lens))
    ref = mha_ref(qkv, lens, ac.HEADS, ac.D, dctx)
    gm = ac.block_gmax(ref[2], lens, ac.HEADS, ac.D)
    assert gm.shape == ref[2].shape and gm[0, 0] == np.abs(ref[2][:250].reshape(250, 3, 3, 64)[:, :, 0]).max()
    # ramp=True never tightens
    a, b = ac.limits("f16", ref, lens, ac.HEADS, ac.D), ac.limits("f16", ref, lens, ac.HEADS, ac.D, ramp=True)
    assert np.all(b[2] >= a[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
