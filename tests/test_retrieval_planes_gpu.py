"""Plane-pair storage of the flat index (FlatIPIndex(storage="planes")) on the GPU: the split on the device,
ip_scores_planes_kernel, ip_filter_planes_kernel and the two searches built on them.  Semantics under test (include/simx.h): a
float32 value is held as hi = rnd16(x), lo = rnd16(x - hi); a score is the float32 MFMA accumulation of
Qhi.Clo + Qlo.Chi + Qhi.Chi in one K loop of fixed order (lo.lo dropped); top-k / ties / padding as the other two modes.

  * grid data (test_retrieval_planes_cpu.grid_emb): every partial sum is exact in any order, so D and I equal the NumPy three-term
    sums bit for bit -- which a kernel that scores hi.hi only, or the full product, does not (checked on the CPU);
  * integer data: lo = 0, the result equals the C oracle's;
  * one-hot queries read float32(hi) + float32(lo) of the corpus back: the split rule and its error model;
  * random float32 data against the float64 product of the ORIGINAL operands:
      bound = (3 H 2^-23 + 2^-21) sum|q c| + sum d(q) |c| + sum |q| d(c),   d(x) = max(2^-22 |x|, 2^-25)
    -- 3 H float32 additions at one unit in the last place of a partial sum that never exceeds sum|q c| (times 1 + 2^-10 for the
    correction terms, inside the 2^-21), the two representation errors, and the dropped lo.lo <= 2^-22 sum|q c| (inside the
    2^-21).  Derived, not measured; a safety net.  The discriminating check is the rms error relative to the float32-chain index
    (storage="fp32") on the same data: at most R_MAX times it.  binary16-only arithmetic gives >= 250 there.
  * fused = unfused bit for bit, and no dependence on chunk or query block."""
import numpy as np
import pytest
import torch

from oracle import retrieval as orr
from test_retrieval_f16_cpu import int_emb
from test_retrieval_planes_cpu import SHAPES, grid_emb, ranked, split16, three_term

pytestmark = pytest.mark.gpu

RANDOM_CASES = [(130, 1000, 768, 200, 1.0), (130, 1000, 768, 200, 0.05), (16, 3000, 128, 10, 1.0), (16, 3000, 128, 10, 0.05)]   # (nq, nc, H, k, scale)
# rms error of the planes index / rms error of the float32-chain index, both against float64.  Measured on the MI355X for the four
# RANDOM_CASES: 0.606, 0.948, 0.595, 1.083; the limit is twice the largest and may never exceed 16
R_MAX = 2.17
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _search(dev, q, c, k, id_base=0, parts=1, storage="planes", fallbacks=0, **kw):
    from simxns_amd.retrieval import FlatIPIndex
    index = FlatIPIndex(q.shape[1], id_base=id_base, storage=storage, **kw)
    for p in range(parts):
        lo, hi = p * len(c) // parts, (p + 1) * len(c) // parts
        index.add(torch.tensor(c[lo:hi]).to(dev))
    assert index.ntotal == len(c)
    D, I = index.search(torch.tensor(q).to(dev), k)
    torch.cuda.synchronize()
    assert index.last_search_fallbacks == fallbacks, "query blocks searched again: %d, expected %d" % (index.last_search_fallbacks, fallbacks)
    return D.cpu().numpy(), I.cpu().numpy()


def _delta(x):
    return np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25)


def _random_case(case):
    """(q, c, ref, bound) of a random case, computed once: ref = the float64 product of the float32 operands, bound as above"""
    if case not in _cache:
        nq, nc, H, k, scale = RANDOM_CASES[case]
        rs = np.random.RandomState(100 + case)
        q, c = (rs.randn(nq, H) * scale).astype(np.float32), (rs.randn(nc, H) * scale).astype(np.float32)
        q64, c64 = q.astype(np.float64), c.astype(np.float64)
        aq, ac = np.abs(q64), np.abs(c64)
        bound = (3 * H * 2.0 ** -23 + 2.0 ** -21) * (aq @ ac.T) + _delta(q64) @ ac.T + aq @ _delta(c64).T
        _cache[case] = (q, c, q64 @ c64.T, bound)
        for a in _cache[case]:
            a.setflags(write=False)
    return _cache[case]


def _grid_case(shape):
    key = ("grid", shape)
    if key not in _cache:
        nq, nc, H, k, chunk = SHAPES[shape]
        q, c = grid_emb(nc, nq, H), grid_emb(nc + 1, nc, H)
        _cache[key] = (q, c) + ranked(three_term(q, c).astype(np.float32), k, id_base=1000)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


# ------------------------------------------------------------------------------------------ 1. exact on grid data
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_grid_data_equals_the_three_term_sums_bit_for_bit(dev, shape):
    nq, nc, H, k, chunk = SHAPES[shape]
    q, c, rd, ri = _grid_case(shape)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, chunk=chunk)
    assert (_bits(D) == _bits(rd)).all(), "scores differ from Qhi.Clo + Qlo.Chi + Qhi.Chi"
    assert (I == ri).all(), "ids differ from the order by (score descending, id ascending)"
    if k > nc:
        assert (I[:, nc:] == -1).all() and np.isneginf(D[:, nc:]).all()


# ------------------------------------------------------------------------------------------ 2. integer data: lo = 0
@pytest.mark.parametrize("nq,nc,H,k,chunk", SHAPES)
def test_integer_data_matches_the_oracle_bit_for_bit(dev, nq, nc, H, k, chunk):
    q, c = int_emb(nc, nq, H), int_emb(nc + 1, nc, H)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, chunk=chunk)
    rd, ri = orr.search(q, c, k, id_base=1000)
    assert (I == ri).all(), "ids differ from the oracle (ties: lower id first)"
    assert (_bits(D) == _bits(rd)).all(), "scores differ from the exact integer sums"


# ------------------------------------------------------------------------------------------ 3. the kernel alone
def test_score_kernel_ragged_tiles_and_leading_dimension(dev):
    """nq, nc no multiples of the tile, H = 72 (one full 64-wide stage + a K tail of 8), ld > nc -- the columns past nc stay
    untouched; a bad H is refused before any launch"""
    from simxns_amd import _lib as L
    from simxns_amd.retrieval import split_planes
    nq, nc, H, ld = 133, 261, 72, 268
    q, c = grid_emb(1, nq, H), grid_emb(2, nc, H)
    qh, ql = split_planes(torch.from_numpy(q).to(dev))
    ch, cl = split_planes(torch.from_numpy(c).to(dev))
    out = torch.full((nq, ld), float("nan"), device=dev)
    L.call("simx_ip_scores_planes", L.stream_ptr(), nq, nc, H, L.ptr(qh), L.ptr(ql), L.ptr(ch), L.ptr(cl), L.ptr(out), ld)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (_bits(got[:, :nc]) == _bits(three_term(q, c).astype(np.float32))).all()
    assert np.isnan(got[:, nc:]).all(), "the kernel wrote past column nc"
    with pytest.raises(L.SimxError):
        L.call("simx_ip_scores_planes", L.stream_ptr(), nq, nc, 12, L.ptr(qh), L.ptr(ql), L.ptr(ch), L.ptr(cl), L.ptr(out), ld)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()[:, nc:]).all()


# ------------------------------------------------------------------------------------------ 4. the split, read back
def test_rows_are_split_into_two_binary16_planes(dev):
    H = 8
    rs = np.random.RandomState(5)
    mag = np.exp2(rs.uniform(-10.0, 15.0, size=(292, H)))                    # 2^-10 .. 2^15: finite and normal in binary16
    c = (mag * rs.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
    t = 2.0 ** -11                                                           # half a unit in the last place at 1.0
    special = np.array([1 + t, 1 + 3 * t, -(1 + t), -(1 + 3 * t), 1 + 5 * t, 1 + 7 * t, 2 + 2 * t, 2 + 6 * t,      # exact halfway cases
                        1 + 0.99 * t, 1 + 1.01 * t, 1024 + 0.5, 1024 + 1.5, 2.0 ** -14 + 2.0 ** -25, 2.0 ** -14 + 3 * 2.0 ** -25,
                        65504.0 - 8.0, 0.1, 1.0 / 3.0, -2.0 / 3.0, 3.14159265, 1e-3, 60000.0, -60000.0, 0.3, 7e-4], np.float32)
    c = np.concatenate([c, np.resize(special, (8, H))], 0)
    hi, lo = split16(c)
    assert np.isfinite(hi).all() and (hi != c).mean() > 0.9 and (lo != 0).mean() > 0.9       # the data needs both planes
    c64 = c.astype(np.float64)
    err = np.abs(c64 - hi.astype(np.float64) - lo.astype(np.float64))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(c64), 2.0 ** -25)).all(), "the error model of the split"
    expect = hi + lo                                                         # float32; exact: hi + lo has at most 24 significant bits
    assert (expect.astype(np.float64) == hi.astype(np.float64) + lo.astype(np.float64)).all()
    nc = len(c)
    D, I = _search(dev, np.eye(H, dtype=np.float32), c, nc)
    S = np.empty((H, nc), np.float32)
    np.put_along_axis(S, I, D, 1)
    assert (np.sort(I, 1) == np.arange(nc)).all()
    assert (_bits(S) == _bits(expect.T)).all(), "score (j, row) must be float32(hi) + float32(lo) of c[row, j]"


# ------------------------------------------------------------------------------------------ 5. random float32 data
@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_random_data_bound_and_error_relative_to_the_float32_chain(dev, case):
    nq, nc, H, k, scale = RANDOM_CASES[case]
    q, c, ref, bound = _random_case(case)
    D, I = _search(dev, q, c, k)
    assert ((I >= 0) & (I < nc)).all(), "invalid id"
    assert (np.diff(np.sort(I, 1), axis=1) > 0).all(), "duplicate id in a row"
    # (a) the derived bound
    err = np.abs(D.astype(np.float64) - np.take_along_axis(ref, I, 1))
    lim = np.take_along_axis(bound, I, 1)
    # (b) against the float32 chain of the default index on the same data
    D32, I32 = _search(dev, q, c, k, storage="fp32")
    err32 = np.abs(D32.astype(np.float64) - np.take_along_axis(ref, I32, 1))
    rms, rms32 = np.sqrt((err ** 2).mean()), np.sqrt((err32 ** 2).mean())
    print("case %r: max |score - ref| = %.3e, max error / bound = %.4f, rms error planes %.3e / fp32 chain %.3e = ratio %.3f"
          % (RANDOM_CASES[case], err.max(), (err / lim).max(), rms, rms32, rms / rms32))
    assert (err <= lim).all(), "score outside the derived bound of the float64 product"
    assert rms32 > 0 and rms <= R_MAX * rms32, "rms error %.3e is more than %g x the float32 chain's %.3e" % (rms, R_MAX, rms32)
    # (c) order
    dd = np.diff(D, axis=1)
    assert (dd <= 0).all(), "scores must be non-increasing"
    assert (np.diff(I, axis=1)[dd == 0] > 0).all(), "equal scores must come in ascending id"
    # (d) membership, the argument of test_retrieval_f16_gpu.py: two scores are compared, so two bounds add up -- the id's own and
    # that of the (unknown) id it displaced or was displaced by, for which the row's largest bound stands
    ref_k = -np.partition(-ref, k - 1, axis=1)[:, k - 1:k]                    # k-th largest reference score per row
    bmax = bound.max(1, keepdims=True)
    assert (np.take_along_axis(ref, I, 1) >= ref_k - (lim + bmax)).all(), "a returned id is not among the best within the bound"
    present = np.zeros((nq, nc), bool)
    np.put_along_axis(present, I, True, 1)
    assert present[ref > ref_k + (bound + bmax)].all(), "an id clearly above the k-th score is missing"


# ------------------------------------------------------------------------------------------ 6. partition independence
def test_scores_do_not_depend_on_chunk_or_query_block(dev):
    nq, nc, H, k, _ = RANDOM_CASES[0]
    q, c, _, _ = _random_case(0)
    D0, I0 = _search(dev, q, c, k, chunk=65536)
    for kw in (dict(chunk=64), dict(chunk=65536, query_block=8), dict(chunk=64, query_block=8)):
        D, I = _search(dev, q, c, k, **kw)
        assert (I == I0).all() and (_bits(D) == _bits(D0)).all(), "result changed with %r" % (kw,)


# ------------------------------------------------------------------------------------------ 7. fused = unfused
# seed rows per shape: k < seed < nc where the shape allows it, so that the later chunks are really filtered; lists <= chunk <= 4096
FUSED_SEED = {1: 256, 2: 1024, 3: 32}


@pytest.mark.parametrize("data", ["random", "grid"])
@pytest.mark.parametrize("shape", [1, 2, 3])
def test_fused_equals_unfused_bit_for_bit(dev, shape, data):
    nq, nc, H, k, chunk = SHAPES[shape]
    if data == "grid":
        q, c, rd, ri = _grid_case(shape)
    else:
        rs = np.random.RandomState(200 + shape)
        q, c = rs.randn(nq, H).astype(np.float32), rs.randn(nc, H).astype(np.float32)
        rd, ri = _search(dev, q, c, k, id_base=1000, chunk=chunk)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, fused=True, seed_rows=FUSED_SEED[shape], chunk=min(chunk, 4096))
    assert (I == ri).all() and (_bits(D) == _bits(rd)).all(), "the one-pass search differs from the unfused one"


def test_fused_ascending_scores_overflow_and_fall_back(dev):
    """corpus row j = (j / 8, 0, ..) against queries (1 + 2^-12, ..) > 0: every row beats all rows before it, so every fused chunk
    lists all its rows (>= 64 > cand_cap = 8), the block is searched again unfused and the result is still the exact one"""
    nq, nc, H, k = 7, 2000, 8, 10
    c = np.zeros((nc, H), np.float32)
    c[:, 0] = np.arange(nc) / 8.0
    q = grid_emb(31, nq, H)
    q[:, 0] = np.abs(q[:, 0])
    rd, ri = ranked(three_term(q, c).astype(np.float32), k, id_base=1000)
    assert (ri == 1000 + nc - 1 - np.arange(k)).all()
    D0, I0 = _search(dev, q, c, k, id_base=1000)
    D, I = _search(dev, q, c, k, id_base=1000, fused=True, seed_rows=64, chunk=128, cand_cap=8, fallbacks=1)
    assert (I == I0).all() and (_bits(D) == _bits(D0)).all(), "the fallback's result differs from the unfused search"
    assert (I == ri).all() and (_bits(D) == _bits(rd)).all()
