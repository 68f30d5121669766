"""The optimizer kernels of csrc/optim.hip through the C ABI: every form an element can be processed in gives the same bits.

AdamW walks a buffer as float4 plus a scalar tail in block 0, LAMB walks a segment as scalar head, float4 body and scalar tail,
and both have a skip path under the loss scaler; the squared norm has an atomic and a deterministic exit and a capped,
grid-striding launch.  Buffers tiled from four base elements make "the update does not depend on where an element sits" a
bit-for-bit statement.  Tolerances are test_adamw_clip's: 1e-3 relative on the norm, rtol 1e-5 / atol 1e-6 against float64."""
import math

import numpy as np
import pytest
import torch

from oracle import optim as ooptim

pytestmark = pytest.mark.gpu
WS_FLOATS = 2048                                  # SIMX_SQNORM_WS_FLOATS of include/simx.h (test_host_cpu.py ties _lib.py to it)
SKIP = [65536.0, 1.0 / 65536.0, 0.0, 1.0, 1.0, 1.0, 2000.0, 2.0 ** 24]      # loss-scaler state with the skip flag [3] set


def L():
    from simxns_amd import _lib
    _lib.load()
    return _lib


def _tiled(n, seed, shift=0):
    """p, g, m, v of n elements, element i holding base[(i - shift) % 4]; v >= 0."""
    rs = np.random.RandomState(seed)
    base = [rs.randn(4).astype(np.float32) * s for s in (1.0, 3.0, 0.1)] + [(rs.randn(4).astype(np.float32) * 0.1) ** 2]
    return [b[(np.arange(n) - shift) % 4].copy() for b in base]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def _sqnorm_det(lib, g, dev):
    sq = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.empty(WS_FLOATS, dtype=torch.float32, device=dev)
    lib.call("simx_sqnorm_accum_det", lib.stream_ptr(), lib.ptr(g), g.numel(), lib.ptr(sq), lib.ptr(ws))
    return sq


def _adamw(lib, name, bufs, sq, max_norm, grad_scale, zero_grad, wd=0.01, step=3, *more):
    p, g, m, v = bufs
    lib.call(name, lib.stream_ptr(), lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), p.numel(), 1e-3, 0.9, 0.999, 1e-8, wd, step,
             lib.ptr(sq), max_norm, grad_scale, zero_grad, *more)
    torch.cuda.synchronize()


class Lamb(object):
    """One segment [1, 1031) of a 1032-element buffer: head 3, body 256 float4, tail 3."""
    n, off, length = 1032, 1, 1030

    def __init__(self, lib, dev):
        from simxns_amd.optim import lamb_chunk_plan
        self.lib, self.dev = lib, dev
        chunks, seg_chunks, seg_range, seg_wd = lamb_chunk_plan([(self.off, self.length, 0.01)], lib.load().simx_lamb_chunk())
        hp = lambda a: a.ctypes.data_as(lib.C.c_void_p)
        lib.call("simx_lamb_plan_check", hp(chunks), len(chunks), hp(seg_chunks), hp(seg_range), 1, self.n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        self.nchunk, self.chunks, self.seg_chunks, self.seg_wd = len(chunks), up(chunks), up(seg_chunks), up(seg_wd)
        self.bufs = [torch.from_numpy(a).to(dev) for a in _tiled(self.n, 5, shift=self.off)]
        self.stats = torch.full((1, 3), float("nan"), dtype=torch.float32, device=dev)
        self.partials = torch.zeros(2 * self.nchunk, dtype=torch.float32, device=dev)

    def step(self, max_norm, zero_grad, scaler=None):
        lib, (p, g, m, v) = self.lib, self.bufs
        sq = _sqnorm_det(lib, g, self.dev)
        lib.call("simx_lamb_step", lib.stream_ptr(), lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), self.n, lib.ptr(self.chunks),
                 self.nchunk, lib.ptr(self.seg_chunks), lib.ptr(self.seg_wd), 1, lib.ptr(self.stats), lib.ptr(self.partials), 1e-3,
                 0.9, 0.999, 1e-6, lib.ptr(sq), max_norm, 1.0, zero_grad, lib.ptr(scaler))
        torch.cuda.synchronize()
        return sq


def test_adamw_position_does_not_matter(dev):
    lib = L()
    n = 1031                                          # 4 * 257 + 3: the tail elements hold the values of elements 0..2
    bufs = [torch.from_numpy(a).to(dev) for a in _tiled(n, 3)]
    sq = _sqnorm_det(lib, bufs[1], dev)
    max_norm = 0.25 * 0.5 * math.sqrt(float(sq))      # a quarter of the norm the kernel sees (grad_scale 0.5): the clip bites
    before = _bits(bufs[0])
    _adamw(lib, "simx_adamw_step", bufs, sq, max_norm, 0.5, 1)
    for t, k in zip((bufs[0], bufs[2], bufs[3]), "pmv"):
        b = _bits(t)
        print("adamw %s: %d elements differ from their float4 twin" % (k, (b != b[np.arange(n) % 4]).sum()))
        assert (b == b[np.arange(n) % 4]).all(), "%s depends on where the element sits" % k
    assert (_bits(bufs[0]) != before).all()
    assert float(bufs[1].abs().max()) == 0.0 and (_bits(bufs[1]) == 0).all()


def test_lamb_position_does_not_matter(dev):
    lib = L()
    f = Lamb(lib, dev)
    before = [_bits(t) for t in f.bufs]
    sq = _sqnorm_det(lib, f.bufs[1], dev)
    f.step(0.25 * math.sqrt(float(sq)), 1)
    seg = np.arange(f.off, f.off + f.length)
    for t, b0, k in zip(f.bufs, before, "pgmv"):
        b = _bits(t)
        assert b[0] == b0[0] and b[-1] == b0[-1], "%s outside the segment changed" % k
        if k == "g":
            assert (b[seg] == 0).all()
        else:
            print("lamb %s: %d elements differ from their float4 twin" % (k, (b[seg] != b[f.off + 4 + (seg - f.off) % 4]).sum()))
            assert (b[seg] == b[f.off + 4 + (seg - f.off) % 4]).all(), "%s depends on where the element sits" % k
            assert (b[seg] != b0[seg]).all()
    assert bool(torch.isfinite(f.stats).all())


def test_adamw_step_is_step_sc_with_a_null_scaler(dev):
    lib = L()
    n = 1031
    rs = np.random.RandomState(7)
    host = [rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32) * 3, rs.randn(n).astype(np.float32) * 0.1,
            (rs.randn(n).astype(np.float32) * 0.1) ** 2]
    out = []
    for name, more in (("simx_adamw_step", ()), ("simx_adamw_step_sc", (None,))):
        bufs = [torch.from_numpy(a.copy()).to(dev) for a in host]
        sq = _sqnorm_det(lib, bufs[1], dev)
        _adamw(lib, name, bufs, sq, 2.0, 1.0, 0, 0.01, 3, *more)
        out.append([_bits(t) for t in bufs])
    assert float(np.sqrt((host[1].astype(np.float64) ** 2).sum())) > 2.0
    for a, b, a0, k in zip(out[0], out[1], host, "pgmv"):
        assert (a == b).all(), k
        assert k == "g" or (a != a0.view(np.int32)).any()


def test_skip_without_zeroing_touches_nothing(dev):
    lib = L()
    sc = torch.tensor(SKIP, dtype=torch.float32, device=dev)
    bufs = [torch.from_numpy(a).to(dev) for a in _tiled(1031, 9)]
    before = [_bits(t) for t in bufs]
    _adamw(lib, "simx_adamw_step_sc", bufs, _sqnorm_det(lib, bufs[1], dev), 1.0, 1.0, 0, 0.01, 3, lib.ptr(sc))
    for t, b, k in zip(bufs, before, "pgmv"):
        assert (_bits(t) == b).all(), "adamw: a skipped step without zero_grad changed %s" % k
    f = Lamb(lib, dev)
    before = [_bits(t) for t in f.bufs + [f.stats]]
    f.step(1.0, 0, scaler=sc)
    for t, b, k in zip(f.bufs + [f.stats], before, "p g m v stats".split()):
        assert (_bits(t) == b).all(), "lamb: a skipped step without zero_grad changed %s" % k


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2098179])       # the last: more than 2048 blocks x 256 threads x 4 elements
def test_sqnorm_all_launch_regimes(dev, n):
    lib = L()
    g = (np.random.RandomState(n % 1000).randn(n) * 3.0).astype(np.float32)
    ref = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    dg = torch.from_numpy(g).to(dev)
    ws = torch.empty(WS_FLOATS, dtype=torch.float32, device=dev)
    det = lambda sq: lib.call("simx_sqnorm_accum_det", lib.stream_ptr(), lib.ptr(dg), n, lib.ptr(sq), lib.ptr(ws))
    atomic = lambda sq: lib.call("simx_sqnorm_accum", lib.stream_ptr(), lib.ptr(dg), n, lib.ptr(sq))
    a, b = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    det(a)
    det(b)
    print("n %d: det %.9g, float64 %.9g" % (n, math.sqrt(float(a)), ref))
    assert (_bits(a) == _bits(b)).all(), "the deterministic norm differs between two calls"
    assert abs(math.sqrt(float(a)) - ref) < 1e-3 * ref
    det(a)
    assert abs(math.sqrt(float(a) / 2.0) - ref) < 1e-3 * ref, "the deterministic entry overwrites its accumulator"
    c = torch.zeros(1, device=dev)
    atomic(c)
    print("n %d: atomic %.9g" % (n, math.sqrt(float(c))))
    assert abs(math.sqrt(float(c)) - ref) < 1e-3 * ref
    atomic(c)
    assert abs(math.sqrt(float(c) / 2.0) - ref) < 1e-3 * ref, "the atomic entry overwrites its accumulator"


def test_adamw_above_its_grid_cap(dev):
    lib = L()
    n = 4195331                                       # 4096 blocks x 256 threads x 4 elements + 1027: grid stride and an odd tail
    rs = np.random.RandomState(11)
    p, g = rs.randn(n).astype(np.float32), (rs.randn(n) * 3.0).astype(np.float32)
    bufs = [torch.from_numpy(a).to(dev) for a in (p, g, np.zeros(n, np.float32), np.zeros(n, np.float32))]
    sq = _sqnorm_det(lib, bufs[1], dev)
    _adamw(lib, "simx_adamw_step", bufs, sq, 2.0, 1.0, 1, 0.01, 1)
    tot, coef = ooptim.clip_coef([g], 2.0)
    P, M, V = p.astype(np.float64), np.zeros(n), np.zeros(n)
    ooptim.adamw_hf_step(P, g.astype(np.float64) * coef, M, V, 1, 1e-3, wd=0.01)
    got = bufs[0].cpu().numpy().astype(np.float64)
    err, lim = np.abs(got - P), 1e-6 + 1e-5 * np.abs(P)
    print("adamw n %d: worst %.4f of the bound" % (n, (err / lim).max()))
    assert (err <= lim).all(), "%d of %d out of tolerance, first at %d" % ((err > lim).sum(), n, int((err > lim).argmax()))
    assert float(bufs[1].abs().max()) == 0.0
