"""float16 storage of the flat index (FlatIPIndex(storage="fp16"), faiss's useFloat16) on the GPU: ip_scores_f16_kernel and
the search built on it.  Semantics under test (include/simx.h): rows and queries rounded to binary16 (nearest even), a score =
the float32 sum of the exact products in one K loop of fixed order, top-k / ties / padding as the float32 index.

  * integer data: every partial sum is exact, so D and I equal the C oracle bit for bit (test_retrieval_f16_cpu.py checks that
    the oracle itself is exact there);
  * rounding: one-hot queries read the rounded corpus back;
  * random data: bound = H * 2^-23 * sum_h |q_h c_h| per score -- the products of two binary16 values are exact in float32 and
    each of the at most H float32 additions errs by at most one unit in the last place of a partial sum that never exceeds
    sum_h |q_h c_h| (2^-23 relative, under any rounding mode).  Derived, not measured."""
import numpy as np
import pytest
import torch

from oracle import retrieval as orr
from test_retrieval_f16_cpu import INT_SHAPES, f16_emb, int_emb

pytestmark = pytest.mark.gpu

RANDOM_SHAPES = [(130, 1000, 768, 200), (16, 3000, 128, 10)]          # (nq, nc, H, k)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _search(dev, q, c, k, id_base=0, parts=1, **kw):
    from simxns_amd.retrieval import FlatIPIndex
    index = FlatIPIndex(q.shape[1], id_base=id_base, storage="fp16", **kw)
    for p in range(parts):
        lo, hi = p * len(c) // parts, (p + 1) * len(c) // parts
        index.add(torch.tensor(c[lo:hi]).to(dev))
    assert index.ntotal == len(c)
    D, I = index.search(torch.tensor(q).to(dev), k)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def _random_case(nq, nc, H):
    """(q, c, ref, bound) of a random shape, computed once: ref = the float64 product, bound as in the module docstring"""
    key = (nq, nc, H)
    if key not in _cache:
        q, c = f16_emb(nq + nc, nq, H), f16_emb(nq + nc + 1, nc, H)
        q64, c64 = q.astype(np.float64), c.astype(np.float64)
        _cache[key] = (q, c, q64 @ c64.T, H * 2.0 ** -23 * (np.abs(q64) @ np.abs(c64).T))
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


# ------------------------------------------------------------------------------------------ 1. exact on integer data
@pytest.mark.parametrize("nq,nc,H,k,chunk", INT_SHAPES)
def test_integer_data_matches_the_oracle_bit_for_bit(dev, nq, nc, H, k, chunk):
    q, c = int_emb(nc, nq, H), int_emb(nc + 1, nc, H)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, chunk=chunk)
    rd, ri = orr.search(q, c, k, id_base=1000)
    assert (I == ri).all(), "ids differ from the oracle (ties: lower id first)"
    assert (_bits(D) == _bits(rd)).all(), "scores differ from the exact integer sums"
    if k > nc:
        assert (I[:, nc:] == -1).all() and np.isneginf(D[:, nc:]).all()


def test_score_kernel_ragged_tiles_and_leading_dimension(dev):
    """the kernel alone: nq, nc no multiples of the tile, H = 72 (one full 64-wide stage + a K tail of 8), ld > nc -- the
    columns past nc stay untouched; a bad H is refused before any launch"""
    from simxns_amd import _lib as L
    nq, nc, H, ld = 133, 261, 72, 268
    q, c = int_emb(1, nq, H), int_emb(2, nc, H)
    tq, tc = torch.from_numpy(q).to(dev).to(torch.float16), torch.from_numpy(c).to(dev).to(torch.float16)
    out = torch.full((nq, ld), float("nan"), device=dev)
    L.call("simx_ip_scores_f16", L.stream_ptr(), nq, nc, H, L.ptr(tq), L.ptr(tc), L.ptr(out), ld)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :nc] == (q.astype(np.float64) @ c.astype(np.float64).T)).all()
    assert np.isnan(got[:, nc:]).all(), "the kernel wrote past column nc"
    with pytest.raises(L.SimxError):
        L.call("simx_ip_scores_f16", L.stream_ptr(), nq, nc, 12, L.ptr(tq), L.ptr(tc), L.ptr(out), ld)


# ------------------------------------------------------------------------------------------ 2. rounding
def test_rows_are_rounded_to_binary16_nearest_even(dev):
    H = 8
    rs = np.random.RandomState(5)
    mag = np.exp2(rs.uniform(-10.0, 15.5, size=(292, H)))                    # 2^-10 .. 4.6e4: finite and normal in binary16
    c = (mag * rs.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
    t = 2.0 ** -11                                                           # half a unit in the last place at 1.0
    special = np.array([1 + t, 1 + 3 * t, -(1 + t), -(1 + 3 * t), 1 + 5 * t, 1 + 7 * t, 2 + 2 * t, 2 + 6 * t,      # exact halfway cases
                        1 + 0.99 * t, 1 + 1.01 * t, 1024 + 0.5, 1024 + 1.5, 2.0 ** -14 + 2.0 ** -25, 2.0 ** -14 + 3 * 2.0 ** -25,
                        65504.0 - 8.0, 0.1, 1.0 / 3.0, -2.0 / 3.0, 3.14159265, 1e-3, 60000.0, -60000.0, 0.3, 7e-4], np.float32)
    c = np.concatenate([c, np.resize(special, (8, H))], 0)
    expect = c.astype(np.float16)
    assert np.isfinite(expect).all() and (np.abs(expect.astype(np.float32)) >= 2.0 ** -14).all()
    assert (expect.astype(np.float32) != c).mean() > 0.9                      # the data is NOT representable
    assert np.float16(np.float32(1 + t)) == 1.0 and np.float16(np.float32(1 + 3 * t)) == np.float16(1 + 4 * t)   # ties to even
    nc = len(c)
    D, I = _search(dev, np.eye(H, dtype=np.float32), c, nc)
    S = np.empty((H, nc), np.float32)
    np.put_along_axis(S, I, D, 1)
    assert (np.sort(I, 1) == np.arange(nc)).all()
    assert (_bits(S) == _bits(expect.astype(np.float32).T)).all(), "score (j, row) must be binary16(c[row, j])"


# ------------------------------------------------------------------------------------------ 3. random data, derived bound
@pytest.mark.parametrize("nq,nc,H,k", RANDOM_SHAPES)
def test_random_data_within_the_derived_bound(dev, nq, nc, H, k):
    q, c, ref, bound = _random_case(nq, nc, H)
    D, I = _search(dev, q, c, k)
    assert ((I >= 0) & (I < nc)).all(), "invalid id"
    assert (np.diff(np.sort(I, 1), axis=1) > 0).all(), "duplicate id in a row"
    err = np.abs(D.astype(np.float64) - np.take_along_axis(ref, I, 1))
    lim = np.take_along_axis(bound, I, 1)
    print("max |score - ref| = %.3e, max error / bound = %.4f" % (err.max(), (err / lim).max()))
    assert (err <= lim).all(), "score outside H * 2^-23 * sum|q c| of the float64 product"
    dd = np.diff(D, axis=1)
    assert (dd <= 0).all(), "scores must be non-increasing"
    assert (np.diff(I, axis=1)[dd == 0] > 0).all(), "equal scores must come in ascending id"
    # membership: two scores are compared, so two bounds add up -- the id's own and that of the (unknown) id it displaced or
    # was displaced by, for which the row's largest bound stands.  A returned i outside the reference's best k displaced some j
    # inside it: ref_i + b_i >= s_i >= s_j >= ref_j - b_j >= ref_k - b_j; an absent i with ref_i > ref_k lost to a returned j with
    # ref_j <= ref_k: ref_i - b_i <= s_i <= s_j <= ref_k + b_j.
    ref_k = -np.partition(-ref, k - 1, axis=1)[:, k - 1:k]                    # k-th largest reference score per row
    bmax = bound.max(1, keepdims=True)
    assert (np.take_along_axis(ref, I, 1) >= ref_k - (lim + bmax)).all(), "a returned id is not among the best within the bound"
    present = np.zeros((nq, nc), bool)
    np.put_along_axis(present, I, True, 1)
    assert present[ref > ref_k + (bound + bmax)].all(), "an id clearly above the k-th score is missing"


# ------------------------------------------------------------------------------------------ 4. partition independence
def test_scores_do_not_depend_on_chunk_or_query_block(dev):
    nq, nc, H, k = RANDOM_SHAPES[0]
    q, c, _, _ = _random_case(nq, nc, H)
    D0, I0 = _search(dev, q, c, k, chunk=4096)
    for kw in (dict(chunk=4096), dict(chunk=64), dict(chunk=4096, query_block=5)):
        D, I = _search(dev, q, c, k, **kw)
        assert (I == I0).all() and (_bits(D) == _bits(D0)).all(), "result changed with %r" % (kw,)


# ------------------------------------------------------------------------------------------ 5. shard merge
def test_shard_merge_equals_global_search(dev):
    from simxns_amd.retrieval import fold_candidates
    nq, nc, H, k, W = 40, 8000, 256, 200, 4
    q, c = int_emb(11, nq, H), int_emb(12, nc, H)
    Ds, Is = [], []
    for r in range(W):
        lo, hi = r * nc // W, (r + 1) * nc // W
        d, i = _search(dev, q, c[lo:hi], k, id_base=lo)
        Ds.append(torch.from_numpy(d).to(dev)); Is.append(torch.from_numpy(i).to(dev))
    D, I = fold_candidates(torch.cat(Ds, 1).contiguous(), torch.cat(Is, 1).contiguous(), k)
    D1, I1 = _search(dev, q, c, k)
    assert (I.cpu().numpy() == I1).all() and (_bits(D.cpu().numpy()) == _bits(D1)).all()
    rd, ri = orr.search(q, c, k)
    assert (I1 == ri).all() and (_bits(D1) == _bits(rd)).all()


# ------------------------------------------------------------------------------------------ 6. default untouched
def test_default_storage_is_still_the_float32_chain(dev):
    from simxns_amd.retrieval import FlatIPIndex
    rs = np.random.RandomState(9)
    nq, nc, H, k = 16, 700, 128, 50
    q, c = rs.randn(nq, H).astype(np.float32), rs.randn(nc, H).astype(np.float32)
    index = FlatIPIndex(H)
    index.add(torch.from_numpy(c).to(dev))
    D, I = index.search(torch.from_numpy(q).to(dev), k)
    torch.cuda.synchronize()
    rd, ri = orr.search(q, c, k)
    assert (I.cpu().numpy() == ri).all() and (_bits(D.cpu().numpy()) == _bits(rd)).all()
