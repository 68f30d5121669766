"""Every attention unit against the float64 reference with the stateless mask (oracle/attention.py::mha_ref), where the older
tests compare kernel with kernel or do not go: dropout on every rung and in the chunked kernels (A), the top resident rung and
the chunked kernels on batches of one long and many short sequences (B), softmax rows whose maximum rises or falls chunk after
chunk, forward and backward (C), the single-query kernels with dropout (D) and the one-wave-per-row kernels at head sizes 32, 96
and 128 (E).

The reference runs on the values the kernel sees (the rounded 16-bit inputs, or the plane values).  The bounds are the existing
ones, see tests/attention_cases.py; tests/test_attention_ref_cpu.py shows that they see a misplaced or unscaled mask.  Outputs
start as NaN, so an element a kernel does not write fails too.  Every test prints its worst err / bound.

Worst err / bound measured on an MI355X (ctx, lse, dqkv; D: ctx, dq, dk|dv), per test and unit:
         f32                planes             bf16               f16                x3
    A    .024 .012 .007     .174 .006 .294     .202 .000 .260     .154 .001 .191     .124 .013 .388
    B    .027 .013 .008     .107 .007 .338     .135 .000 .113     .100 .001 .086     .072 .015 .454
    C    .457 .043 .065     .524 .020 .407     .167 .001 .462     .204 .004 .470     .543 .009 .350
    D    .008 .001 .001                        .099 .023 .052     .109 .020 .039
    E    .052 .011 .012                        .102 .000 .133     .101 .001 .193
(C, planes, ctx: 1.047 of the x3 bound it started with, see attention_cases.limits.)  No kernel defect was found.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attention_cases as ac
from tests.test_planes_gpu import planes_of, planes_value, L, F16, BF16

pytestmark = pytest.mark.gpu

UNITS = ["f32", "planes", "bf16", "f16", "x3"]
KIND = {"f32": "f32", "planes": "planes", "bf16": "bf16", "f16": "f16", "x3": "pair"}   # whose bounds
SEES = {"f32": "f32", "planes": "f32", "bf16": "bf16", "f16": "f16", "x3": "x3"}       # which input values


def _nan_pair(rows, cols, dev):
    return torch.full((2, rows, cols), -1, device=dev, dtype=torch.int16)              # 0xFFFF: NaN in fp16 and in bf16


def _f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def run_unit(unit, dev, qkv, dctx, lens, heads, d, drop):
    """forward, then backward on the forward's own ctx and lse -> (qkv seen, dctx seen), (ctx, lse, dqkv), all float64"""
    lib = L()
    T, H, n, S = sum(lens), heads * d, len(lens), max(lens)
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
    dr = C.byref(drop) if drop is not None else None
    lse = torch.full((heads, T), float("nan"), device=dev)
    if unit in ("f32", "bf16", "f16"):
        dt, code = ac.TORCH_DT[unit], ac.CODE[unit]
        q, g = torch.from_numpy(qkv).to(dev).to(dt), torch.from_numpy(dctx).to(dev).to(dt)
        ctx = torch.full((T, H), float("nan"), device=dev, dtype=dt)
        dqkv = torch.full((T, 3 * H), float("nan"), device=dev, dtype=dt)
        lib.call("simx_mha_fwd_ex", lib.stream_ptr(), code, n, heads, d, lib.ptr(cu), S, T, lib.ptr(q), lib.ptr(ctx), lib.ptr(lse), dr)
        lib.call("simx_mha_bwd_ex", lib.stream_ptr(), code, n, heads, d, lib.ptr(cu), S, T, lib.ptr(q), lib.ptr(ctx), lib.ptr(lse),
                 lib.ptr(g), lib.ptr(dqkv), dr)
        torch.cuda.synchronize()
        return (_f64(q), _f64(g)), (_f64(ctx), _f64(lse), _f64(dqkv))
    q, g = torch.from_numpy(qkv).to(dev), torch.from_numpy(dctx).to(dev)
    ctxp, dqkvp = _nan_pair(T, H, dev), _nan_pair(T, 3 * H, dev)
    if unit == "planes":
        lib.call("simx_mha_fwd_planes", lib.stream_ptr(), n, heads, d, lib.ptr(cu), S, T, lib.ptr(q), lib.ptr(ctxp), T * H, lib.ptr(lse), dr)
        lib.call("simx_mha_bwd_planes", lib.stream_ptr(), n, heads, d, lib.ptr(cu), S, T, lib.ptr(q), lib.ptr(ctxp), T * H, lib.ptr(lse),
                 lib.ptr(g), lib.ptr(dqkvp), T * 3 * H, dr)
        seen = _f64(q)
    else:
        qp = planes_of(q, F16, dev)
        lib.call("simx_mha_fwd_x3", lib.stream_ptr(), n, heads, d, lib.ptr(cu), S, T, lib.ptr(qp), T * 3 * H, lib.ptr(ctxp), T * H,
                 lib.ptr(lse), dr)
        lib.call("simx_mha_bwd_x3_bias", lib.stream_ptr(), n, heads, d, lib.ptr(cu), S, T, lib.ptr(qp), T * 3 * H, lib.ptr(ctxp), T * H,
                 lib.ptr(lse), lib.ptr(g), lib.ptr(dqkvp), T * 3 * H, dr, None)
        seen = planes_value(qp, F16)
    torch.cuda.synchronize()
    return (seen, _f64(g)), (planes_value(ctxp, F16), _f64(lse), planes_value(dqkvp, BF16))


def check(tag, got, ref, lim, names=("ctx", "lse", "dqkv")):
    """every element of every output inside its limit (a NaN is outside); prints the worst err / bound of each output"""
    ratios = [ac.worst(g, r, l) for g, r, l in zip(got, ref, lim)]
    print("%-44s err/bound: %s" % (tag, "  ".join("%s %.3f" % (nm, x) for nm, x in zip(names, ratios))))
    for nm, g, r, l in zip(names, got, ref, lim):
        err = np.abs(g - r)
        bad = ~(err <= l)
        if bad.any():
            at = np.unravel_index(np.nanargmax(np.where(bad, np.nan_to_num(err / l, nan=np.inf), 0.0)), err.shape)
            rows = np.unique(np.nonzero(bad)[0 if nm != "lse" else 1])
            raise AssertionError("%s %s: %d/%d outside, worst err/bound %.3f (err %.3e, ref %.3e) at %s; %d rows from %d to %d: %s" % (
                tag, nm, bad.sum(), bad.size, (err / l)[at], err[at], r[at], at, rows.size, rows[0], rows[-1], rows[:12]))


def full_case(unit, dev, name, p=0.0, ramp=None):
    lens = ac.LISTS[name]
    lib = L()
    qkv, dctx = ac.inputs(lens, ramp=ramp)
    drop = lib.Dropout(p, ac.SEED, ac.STREAM) if p else None
    (sq, sg), got = run_unit(unit, dev, qkv, dctx, lens, ac.HEADS, ac.D, drop)
    ref = ac.reference((name, SEES[unit], p, ramp), sq, lens, ac.HEADS, ac.D, sg, (p, ac.SEED, ac.STREAM) if p else None)
    lim = ac.limits(KIND[unit], ref, lens, ac.HEADS, ac.D, ac.drop_k(p) if p else 1.0, ramp=ramp is not None)
    check("%s %s p=%g%s" % (unit, name, p, " ramp " + ramp if ramp else ""), got, ref, lim)


# ------------------------------------------------------------------------------------------ A: dropout against float64
@pytest.mark.parametrize("name,p", [(nm, 0.1) for nm in ac.LISTS] + [("R16", 0.5), ("LONG", 0.5)])     # p = 0.5: thr = 128, scale exactly 2
@pytest.mark.parametrize("unit", UNITS)
def test_dropout_against_float64(dev, unit, name, p):
    """ctx, dq, dk, dv with the mask at row = h * T + token, col = key and its 1 / (1 - p) on P and on dP; lse of the undropped row"""
    full_case(unit, dev, name, p)


# ------------------------------------------------------------------------------------------ B: ragged rungs
@pytest.mark.parametrize("name", ["R10", "R16", "LONG"])
@pytest.mark.parametrize("unit", UNITS)
def test_ragged_rungs(dev, unit, name):
    """one long sequence and many short ones: key tiles wholly beyond len and query tiles without rows on the largest LDS images"""
    full_case(unit, dev, name)


# ------------------------------------------------------------------------------------------ C: key ramps
@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("name", ["R16", "LONG", "LONG2"])
@pytest.mark.parametrize("unit", UNITS)
def test_key_ramps(dev, unit, name, direction):
    """skewed softmax rows, forward and backward: the row maximum in the last (up) or first (down) keys"""
    full_case(unit, dev, name, ramp=direction)


# ------------------------------------------------------------------------------------------ D: single query with dropout
@pytest.mark.parametrize("heads,d,lens", [(3, 64, [160, 129, 45, 300, 1]), (4, 16, [5, 32, 17, 1])])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_single_query_dropout(dev, fmt, heads, d, lens):
    """simx_mha_cls_fwd / _bwd with dropout: the full attention's mask row of token 0.  Reference = mha_ref with dctx zero outside
    the first rows; the Q columns of the packed rows are neither read nor written (as in test_mha_single_query)."""
    lib = L()
    T, H, n = sum(lens), heads * d, len(lens)
    qkv, dcc = ac.rnd((T, 3 * H), 11), ac.rnd((n, H), 12)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    first = cu[:-1]
    qkv_in = qkv.copy()
    qkv_in[:, :H] = 7.0                          # the Q columns of the packed rows must not be read
    dt, code = ac.TORCH_DT[fmt], ac.CODE[fmt]
    dev_of = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    d_qkv, d_qc, d_dcc, dcu = dev_of(qkv_in), dev_of(qkv[first, :H]), dev_of(dcc), torch.from_numpy(cu).to(dev)
    drop = lib.Dropout(0.1, ac.SEED, ac.STREAM)
    ctxc = torch.full((n, H), float("nan"), device=dev, dtype=dt)
    lib.call("simx_mha_cls_fwd", lib.stream_ptr(), code, n, heads, d, lib.ptr(dcu), max(lens), T, lib.ptr(d_qc), lib.ptr(d_qkv),
             lib.ptr(ctxc), C.byref(drop))
    dqc = torch.full((n, H), float("nan"), device=dev, dtype=dt)
    dqkv = torch.full((T, 3 * H), float("nan"), device=dev, dtype=dt)
    dqkv[:, :H] = 3.0
    lib.call("simx_mha_cls_bwd", lib.stream_ptr(), code, n, heads, d, lib.ptr(dcu), max(lens), T, lib.ptr(d_qc), lib.ptr(d_qkv),
             lib.ptr(d_dcc), lib.ptr(dqc), lib.ptr(dqkv), C.byref(drop))
    torch.cuda.synchronize()
    dctx = np.zeros((T, H))
    dctx[first] = ac.rounded(dcc, fmt)
    ref = ac.mha_ref(ac.rounded(qkv, fmt), lens, heads, d, dctx, (0.1, ac.SEED, ac.STREAM))
    lc, _, lq = ac.limits(fmt, ref, lens, heads, d, ac.drop_k(0.1))
    got = _f64(dqkv)
    check("cls %s heads %d d %d" % (fmt, heads, d), (_f64(ctxc), _f64(dqc), got[:, H:]), (ref[0][first], ref[2][first, :H], ref[2][:, H:]),
          (lc[first], lq[first, :H], lq[:, H:]), names=("ctx", "dq", "dkdv"))
    assert np.all(got[:, :H] == 3.0)             # the Q columns of dqkv are left alone


# ------------------------------------------------------------------------------------------ E: the one-wave-per-row kernels
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [32, 96, 128])                      # 96: a lane loop with a ragged last pass; 128: the declared limit
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_fallback_kernels(dev, fmt, d, p):
    """mha_fwd_simple / mha_bwd_simple (every head size but 64), with and without dropout"""
    lib = L()
    heads, lens = 2, [40, 7, 130, 1]
    qkv, dctx = ac.inputs(lens, heads, d)
    drop = lib.Dropout(p, ac.SEED, ac.STREAM) if p else None
    (sq, sg), got = run_unit(fmt, dev, qkv, dctx, lens, heads, d, drop)
    ref = ac.mha_ref(sq, lens, heads, d, sg, (p, ac.SEED, ac.STREAM) if p else None)
    check("simple %s d %d p=%g" % (fmt, d, p), got, ref, ac.limits(fmt, ref, lens, heads, d, ac.drop_k(p) if p else 1.0))
