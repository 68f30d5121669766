"""The fp32 engine's plane-operand GEMMs (csrc/gemm_xp.hip) through the C ABI against float64 NumPy on the same inputs.

A plane pair is hi = rnd16(x), lo = rnd16(x - hi); the kernels compute hi.lo + lo.hi + hi.hi in f32 accumulators, i.e. the
product of the f32 operands up to the split's 2^-22 (fp16 planes, forward) / 2^-17 (bf16 planes, backward) per element and f32
accumulation -- the tolerances below are those figures times the row scale, NOT 16-bit tolerances.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import bert as obert
from oracle import planes as oplanes

pytestmark = pytest.mark.gpu
F32, BF16, F16 = 0, 1, 2


def L():
    from simxns_amd import _lib
    return _lib


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32)


def planes_of(x, fmt, dev):
    """plane pair of an f32 device matrix via simx_planes_from: int16 tensor [2, rows, cols]"""
    lib = L()
    rows, cols = x.shape
    p = torch.empty(2, rows, cols, device=dev, dtype=torch.int16)
    lib.call("simx_planes_from", lib.stream_ptr(), F32, fmt, rows, cols, lib.ptr(x), cols, 0, lib.ptr(p), cols, rows * cols)
    return p


def planes_value(p, fmt):
    """float64 value hi + lo of a plane pair"""
    t = torch.float16 if fmt == F16 else torch.bfloat16
    v = p.view(t).to(torch.float64)
    return (v[0] + v[1]).cpu().numpy()


@pytest.mark.parametrize("fmt", [F16, BF16])
def test_planes_roundtrip(dev, fmt):
    lib = L()
    x = torch.from_numpy(rnd((300, 136), 1) * np.exp(rnd((300, 136), 2) * 2)).to(dev)
    p = planes_of(x, fmt, dev)
    v = planes_value(p, fmt)
    xr = x.cpu().numpy().astype(np.float64)
    rel = 2.0 ** -21 if fmt == F16 else 2.0 ** -16
    assert np.all(np.abs(v - xr) <= rel * np.abs(xr) + (2.0 ** -24 if fmt == F16 else 0.0))
    back = torch.empty_like(x)
    lib.call("simx_planes_join", lib.stream_ptr(), fmt, 300, 136, lib.ptr(p), 136, 300 * 136, lib.ptr(back), 136)
    assert np.array_equal(back.cpu().numpy().astype(np.float64), v.astype(np.float32).astype(np.float64))
    # pair -> pair of the other format
    other = BF16 if fmt == F16 else F16
    q = torch.empty_like(p)
    lib.call("simx_planes_from", lib.stream_ptr(), fmt, other, 300, 136, lib.ptr(p), 136, 300 * 136, lib.ptr(q), 136, 300 * 136)
    w = planes_value(q, other)
    rel2 = 2.0 ** -21 if other == F16 else 2.0 ** -16
    assert np.all(np.abs(w - v) <= rel2 * np.abs(v) + 2.0 ** -24)


NT_CASES = [  # (variant, fmt)
    ("bias", F16), ("bias+res", F16), ("bias+res+drop", F16), ("gelu", F16), ("gelu_infer", F16),
    ("plain", BF16), ("res", BF16), ("dgelu", BF16)]


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 768), (1024, 256, 192), (2048, 2304, 768), (768, 768, 3072),
                                   (66048, 768, 256)])     # the last: 774 tiles on 256 workgroups -- the persistent walk, ragged last round
@pytest.mark.parametrize("variant,fmt", NT_CASES)
def test_gemm_nt_planes(dev, M, N, K, variant, fmt):
    lib = L()
    sa, sb = (0.5, 0.05) if fmt == F16 else (1e-3, 0.05)        # backward operands are small: gradients
    A = torch.from_numpy(rnd((M, K), 1, sa)).to(dev)
    B = torch.from_numpy(rnd((N, K), 2, sb)).to(dev)
    Ap, Bp = planes_of(A, fmt, dev), planes_of(B, fmt, dev)
    bias = torch.from_numpy(rnd((N,), 3, 0.5)).to(dev) if variant.startswith(("bias", "gelu")) else None
    need_in = "res" in variant or variant == "dgelu"
    inn = torch.from_numpy(rnd((M, N), 4)).to(dev) if need_in else None
    Cc = torch.full((M, N), float("nan"), device=dev) if variant not in ("dgelu", "gelu_infer") else None
    Cp = torch.zeros(2, M, N, device=dev, dtype=torch.int16) if variant in ("gelu", "gelu_infer", "dgelu") else None
    epi = {"gelu": 1, "gelu_infer": 3, "dgelu": 2}.get(variant, 0)
    drop = lib.Dropout(0.1, 1234, 7) if variant.endswith("drop") else None
    lib.call("simx_gemm_nt_planes", lib.stream_ptr(), fmt, epi, M, N, K, lib.ptr(Ap), K, M * K, lib.ptr(Bp), K, N * K, lib.ptr(Cc), N,
             lib.ptr(bias), lib.ptr(inn), N, lib.ptr(Cp), N, M * N, C.byref(drop) if drop else None)
    torch.cuda.synchronize()
    Av, Bv = planes_value(Ap, fmt), planes_value(Bp, fmt)
    acc = Av @ Bv.T
    scale = np.sqrt((Av ** 2).sum(1))[:, None] * np.sqrt((Bv ** 2).sum(1))[None, :]      # |a||b| bounds every partial sum
    if bias is not None:
        acc = acc + bias.cpu().numpy().astype(np.float64)
    tol = 2e-6 * scale + 3e-7 * np.abs(acc) + 1e-30           # f32 accumulation over K + the dropped lo.lo term (2^-22 x 2^-22)
    if variant in ("bias", "plain"):
        got = Cc.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - acc) <= tol), np.abs(got - acc).max()
    elif variant in ("bias+res", "res"):
        got = Cc.cpu().numpy().astype(np.float64)
        ref = acc + inn.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - ref) <= tol + 2e-7 * np.abs(ref)), np.abs(got - ref).max()
    elif variant == "bias+res+drop":
        got = Cc.cpu().numpy().astype(np.float64)
        mask = obert.drop_multipliers(0.1, 1234, 7, np.arange(M), np.arange(N))
        ref = acc * mask + inn.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - ref) <= tol * 1.2 + 2e-7 * np.abs(ref)), np.abs(got - ref).max()
    elif variant in ("gelu", "gelu_infer"):
        h = planes_value(Cp, F16)
        assert np.all(np.abs(h - obert.gelu(acc)) <= tol * 1.2 + 6e-7 * np.abs(acc) + 3e-7), np.abs(h - obert.gelu(acc)).max()
        if variant == "gelu":
            d = Cc.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(d - obert.gelu_grad(acc)) <= tol * 1.5 + 1e-6), np.abs(d - obert.gelu_grad(acc)).max()
    else:
        du = planes_value(Cp, BF16)
        ref = acc * inn.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(du - ref) <= (tol + 3e-7 * np.abs(acc)) * np.abs(inn.cpu().numpy()) + 2.0 ** -15 * np.abs(ref)), np.abs(du - ref).max()


@pytest.mark.parametrize("M,N,K", [(256, 256, 2048), (768, 768, 4096), (2304, 768, 4100), (768, 3072, 8192 + 33), (520, 264, 1000),
                                   (768, 768, 40)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_gemm_tn_planes(dev, M, N, K, with_bias, accumulate):
    lib = L()
    A = torch.from_numpy(rnd((K, M), 1, 1e-3) * np.exp(rnd((K, 1), 5, 2.0))).to(dev)          # dY: rows of very different size
    B = torch.from_numpy(rnd((K, N), 2, 0.7)).to(dev)
    Ap, Bp = planes_of(A, BF16, dev), planes_of(B, BF16, dev)
    C0 = rnd((M, N), 3, 0.01)
    Cc = torch.from_numpy(C0.copy()).to(dev)
    db0 = rnd((M,), 4, 0.01)
    db = torch.from_numpy(db0.copy()).to(dev) if with_bias else None
    wsb = lib.load().simx_gemm_tn_planes_workspace_bytes(M, N, K)
    ws = torch.empty(max(wsb, 16) // 4, device=dev)
    lib.call("simx_gemm_tn_planes", lib.stream_ptr(), M, N, K, lib.ptr(Ap), M, K * M, lib.ptr(Bp), N, K * N, lib.ptr(Cc), N, accumulate,
             lib.ptr(ws), wsb, lib.ptr(db))
    torch.cuda.synchronize()
    Av, Bv = planes_value(Ap, BF16), planes_value(Bp, BF16)
    ref = Av.T @ Bv + (C0.astype(np.float64) if accumulate else 0.0)
    scale = np.sqrt((Av ** 2).sum(0))[:, None] * np.sqrt((Bv ** 2).sum(0))[None, :]
    got = Cc.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= 3e-5 * scale + 1e-6 * np.abs(ref)), (np.abs(got - ref) / (scale + 1e-30)).max()
    if with_bias:
        rb = Av.sum(0) + db0.astype(np.float64)
        gb = db.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(gb - rb) <= 1e-5 * np.abs(Av).sum(0) + 1e-7), np.abs(gb - rb).max()


@pytest.mark.parametrize("M,N,K,valid", [(512, 768, 768, 512), (2048, 3072, 768, 1999), (66048, 768, 256, 65900)])
def test_gemm_nt_planes_dgelu_colsum(dev, M, N, K, valid):
    """SIMX_EPI_DGELU with the fused bias gradient: colsum[N] += column sums of (acc * in) over the rows below `valid` (rows past
    the real tokens hold garbage in the engine: here NaN, which must not leak)."""
    lib = L()
    A = torch.from_numpy(rnd((M, K), 1, 1e-3)).to(dev)
    A[valid:] = float("nan")
    B = torch.from_numpy(rnd((N, K), 2, 0.05)).to(dev)
    Ap, Bp = planes_of(A, BF16, dev), planes_of(B, BF16, dev)
    inn = torch.from_numpy(rnd((M, N), 4)).to(dev)
    Cp = torch.zeros(2, M, N, device=dev, dtype=torch.int16)
    cs0 = rnd((N,), 6, 1e-3)
    cs = torch.from_numpy(cs0.copy()).to(dev)
    lib.call("simx_gemm_nt_planes_cs", lib.stream_ptr(), BF16, 2, M, N, K, lib.ptr(Ap), K, M * K, lib.ptr(Bp), K, N * K, None, N,
             None, lib.ptr(inn), N, lib.ptr(Cp), N, M * N, None, lib.ptr(cs), valid)
    torch.cuda.synchronize()
    Av, Bv = planes_value(Ap, BF16)[:valid], planes_value(Bp, BF16)
    ref = (Av @ Bv.T) * inn.cpu().numpy().astype(np.float64)[:valid]
    du = planes_value(Cp, BF16)[:valid]
    scale = np.sqrt((Av ** 2).sum(1))[:, None] * np.sqrt((Bv ** 2).sum(1))[None, :] * np.abs(inn.cpu().numpy().astype(np.float64)[:valid])
    assert np.all(np.abs(du - ref) <= 2.0 ** -15 * np.abs(ref) + 2e-6 * scale + 1e-12)
    got = cs.cpu().numpy().astype(np.float64)
    want = ref.sum(0) + cs0
    assert np.isfinite(got).all()
    assert np.all(np.abs(got - want) <= 2e-5 * np.abs(ref).sum(0) + 1e-7), np.abs(got - want).max()


@pytest.mark.parametrize("rows,cols", [(768, 3072), (2304, 768), (64, 64), (96, 40), (33, 7)])
def test_split_weight_forms(dev, rows, cols):
    """simx_split_weight (what simx_bert_cast_weights runs per dense weight of an fp32 tower): the fp16 plane pair of W, the bf16
    plane pair of W^T and W^T in f32 are BIT-identical to the elementwise definition hi = rnd16(w), lo = rnd16(w - hi) -- on the
    64 x 64-tile kernel (rows, cols multiples of 64) and on the 32 x 32 kernel for every other shape; and the rate of the former."""
    lib = L()
    w = torch.from_numpy(rnd((rows, cols), 7, 0.05) * np.exp(rnd((rows, cols), 8) * 1.5)).to(dev)
    ph = torch.full((2, rows, cols), -1, device=dev, dtype=torch.int16)
    pt = torch.full((2, cols, rows), -1, device=dev, dtype=torch.int16)
    wT = torch.full((cols, rows), float("nan"), device=dev)
    run = lambda: lib.call("simx_split_weight", lib.stream_ptr(), lib.ptr(w), rows, cols, lib.ptr(ph), lib.ptr(pt), lib.ptr(wT))
    run()
    torch.cuda.synchronize()
    assert torch.equal(wT, w.t().contiguous())
    for planes, src, t in ((ph, w, torch.float16), (pt, w.t().contiguous(), torch.bfloat16)):
        hi, lo = (p.to(dev) for p in oplanes.split16(src, t))
        assert torch.equal(planes[0].view(t), hi) and torch.equal(planes[1].view(t), lo)
    # any output may be absent
    ph.fill_(-1)
    lib.call("simx_split_weight", lib.stream_ptr(), lib.ptr(w), rows, cols, lib.ptr(ph), None, None)
    torch.cuda.synchronize()
    assert torch.equal(ph[0].view(torch.float16), w.to(torch.float16))
    if rows * cols >= 768 * 3072:
        from tests.test_attention_x3_gpu import _ms
        ms = _ms(run, 20)
        gbs = rows * cols * 16 / ms / 1e6
        print("split_weight %d x %d: %.3f ms = %.0f GB/s" % (rows, cols, ms, gbs))
        assert gbs > 1000, gbs                       # (the 32 x 32 scalar-store kernel ran at 220 GB/s)


# ------------------------------------------------------------------------------------------ pair outputs against their f32 twins
# A kernel that can leave the same f32 value either as f32 or as a plane pair must leave EXACTLY oracle.planes.split16 of the f32
# form: these pin the bits of pair outputs that the tests above compare for accuracy only.
def assert_pair_bits(planes, v, fmt):
    """int16 device tensor [2, rows, cols] == the plane pair of the f32 tensor v, bit for bit"""
    hi, lo = oplanes.split16(v, fmt)
    assert torch.equal(planes[0].cpu(), hi.view(torch.int16)), "hi plane"
    assert torch.equal(planes[1].cpu(), lo.view(torch.int16)), "lo plane"


# (256, 256, 128 / 192): the smallest shapes simx_gemm_nt_planes_ok accepts, an even and an odd stage count.  512 x 768 is six
# tiles, one per workgroup on any chip (the grid is never below 8 workgroups), so the last case gives the launch a budget of 8 CUs:
# 12 tiles on 8 workgroups, i.e. the persistent loop runs a second tile in half of them.
@pytest.mark.parametrize("M,N,K,cus", [(256, 256, 128, 0), (256, 256, 192, 0), (512, 768, 256, 0), (1024, 768, 256, 8)])
def test_gemm_nt_planes_pair_is_the_split_of_the_f32_twin(dev, M, N, K, cus):
    """gemm_nt_xp_kernel: SIMX_EPI_NONE_PLANES (pair out) == split16 of SIMX_EPI_NONE (f32 C), same fp16 operand planes and bias"""
    lib = L()
    Ap = planes_of(torch.from_numpy(rnd((M, K), 1, 0.5)).to(dev), F16, dev)
    Bp = planes_of(torch.from_numpy(rnd((N, K), 2, 0.05)).to(dev), F16, dev)
    bias = torch.from_numpy(rnd((N,), 3, 0.5)).to(dev)
    Cc = torch.full((M, N), float("nan"), device=dev)
    Cp = torch.full((2, M, N), -1, device=dev, dtype=torch.int16)
    try:
        lib.call("simx_set_compute_cus", cus)
        for epi, c, cp in ((0, Cc, None), (4, None, Cp)):
            lib.call("simx_gemm_nt_planes", lib.stream_ptr(), F16, epi, M, N, K, lib.ptr(Ap), K, M * K, lib.ptr(Bp), K, N * K, lib.ptr(c), N,
                     lib.ptr(bias), None, N, lib.ptr(cp), N, M * N, None)
        torch.cuda.synchronize()
    finally:
        lib.call("simx_set_compute_cus", 0)
    assert torch.isfinite(Cc).all()
    assert_pair_bits(Cp, Cc, "f16")


# 1, 17 and 40 tokens in one batch: the resident kernel; 257: the first length simx_mha_fwd_f32 gives to its _long kernel
# (max_len > 256, csrc/attention_f32.hip).  The backward has no such twin: its PL form reads ctx from the pair.
@pytest.mark.parametrize("lens", [[1, 17, 40], [257]])
def test_mha_fwd_f32_pair_is_the_split_of_the_f32_twin(dev, lens):
    """mha_fwd_f32_kernel / mha_fwd_f32_long_kernel: the PL form's fp16 pair == split16 of the plain form's f32 ctx; equal lse"""
    lib = L()
    heads, d, T = 2, 64, sum(lens)
    H = heads * d
    qkv = torch.from_numpy(rnd((T, 3 * H), 1)).to(dev)
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
    ctx = torch.full((T, H), float("nan"), device=dev)
    ctxp = torch.full((2, T, H), -1, device=dev, dtype=torch.int16)
    lse, lse2 = torch.full((heads, T), float("nan"), device=dev), torch.full((heads, T), float("nan"), device=dev)
    lib.call("simx_mha_fwd_ex", lib.stream_ptr(), F32, len(lens), heads, d, lib.ptr(cu), max(lens), T, lib.ptr(qkv), lib.ptr(ctx), lib.ptr(lse), None)
    lib.call("simx_mha_fwd_planes", lib.stream_ptr(), len(lens), heads, d, lib.ptr(cu), max(lens), T, lib.ptr(qkv), lib.ptr(ctxp), T * H,
             lib.ptr(lse2), None)
    torch.cuda.synchronize()
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert_pair_bits(ctxp, ctx, "f16")
    assert torch.equal(lse, lse2)


def test_planes_from_pair_to_pair_is_split_of_join(dev):
    """planes_kernel pair -> pair (plane_ld8 then plane_split2): fp16 pair -> bf16 pair == split16(join(hi, lo), bf16)"""
    lib = L()
    rows, cols = 37, 72
    rs = np.random.RandomState(11)
    x = (rs.choice([-1.0, 1.0], size=(rows, cols)) * 2.0 ** rs.uniform(-8, 8, size=(rows, cols))).astype(np.float32)
    p = planes_of(torch.from_numpy(x).to(dev), F16, dev)
    q = torch.full((2, rows, cols), -1, device=dev, dtype=torch.int16)
    lib.call("simx_planes_from", lib.stream_ptr(), F16, BF16, rows, cols, lib.ptr(p), cols, rows * cols, lib.ptr(q), cols, rows * cols)
    torch.cuda.synchronize()
    assert_pair_bits(q, oplanes.join(p[0].view(torch.float16), p[1].view(torch.float16)), "bf16")
