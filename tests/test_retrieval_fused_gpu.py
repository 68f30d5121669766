"""One-pass float16 search of the flat index (FlatIPIndex(storage="fp16", fused=True)) on the GPU: ip_filter_f16_kernel, the
list fold of topk_stream_kernel and the chunk schedule of simx_flat_ip_search_f16_fused.

What is claimed (include/simx.h): a score has the bits of the unfused float16 kernel, the filter drops only what cannot enter
the top-k and the fold is the exact top-k, so the fused result equals the unfused one BIT FOR BIT whatever seed_rows, chunk,
cand_cap and query_block are; a candidate list that overflows is counted, and the query block is searched again unfused.

The caps of the tables below come from a CPU simulation of the filter on exactly this data (the schedule: min(seed_rows, nc)
rows unfused, then chunks of min(chunk, rows seen, rows left); a row survives if its score is strictly above the k-th best of
the rows before its chunk); the largest list any (query, chunk) produces is noted next to each cap.  Every search asserts
last_search_fallbacks == 0 unless it is about the fallback, so it is the fused path that is compared."""
import numpy as np
import pytest
import torch

from oracle import retrieval as orr
from test_retrieval_f16_cpu import f16_emb, int_emb

pytestmark = pytest.mark.gpu

# (nq, nc, H, k, seed_rows, chunk, cand_cap, seeds of q / c)                      simulated maximum list
RANDOM_CASES = [(130, 20000, 64, 50, 512, 4096, 256, 1, 2),                     # 86
                (33, 30000, 128, 200, 1024, 8192, 512, 3, 4)]                   # 243
INTEGER_CASES = [(64, 20000, 768, 200, 1024, 4096, 512, 5, 6),                  # 241
                 (7, 3000, 8, 10, 128, 512, 32, 7, 8)]                          # 16
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _search(dev, q, c, k, id_base=0, parts=1, fallbacks=0, **kw):
    """-> (D, I) of a float16 index over c; with fused=True in kw the number of redone query blocks is asserted"""
    from simxns_amd.retrieval import FlatIPIndex
    index = FlatIPIndex(q.shape[1], id_base=id_base, storage="fp16", **kw)
    for p in range(parts):
        lo, hi = p * len(c) // parts, (p + 1) * len(c) // parts
        if hi > lo:
            index.add(torch.tensor(c[lo:hi]).to(dev))
    assert index.ntotal == len(c)
    D, I = index.search(torch.tensor(q).to(dev), k)
    torch.cuda.synchronize()
    assert index.last_search_fallbacks == fallbacks, "query blocks searched again: %d, expected %d" % (index.last_search_fallbacks, fallbacks)
    return D.cpu().numpy(), I.cpu().numpy()


def _random_case(dev, case):
    """(q, c, D, I) of RANDOM_CASES[case], D / I = the UNFUSED float16 search (id_base 1000), computed once"""
    if case not in _cache:
        nq, nc, H, k, _, _, _, sq, sc = RANDOM_CASES[case]
        q, c = f16_emb(sq, nq, H), f16_emb(sc, nc, H)
        _cache[case] = (q, c) + _search(dev, q, c, k, id_base=1000)
        for a in _cache[case]:
            a.setflags(write=False)
    return _cache[case]


def _same(D, I, rd, ri, what):
    assert (I == ri).all(), "%s: ids differ (%d of %d)" % (what, (I != ri).sum(), I.size)
    assert (_bits(D) == _bits(rd)).all(), "%s: score bits differ" % what


# ------------------------------------------------------------------------------------------ 1. random data: fused == unfused
@pytest.mark.parametrize("case", [0, 1])
def test_random_data_equals_the_unfused_search_bit_for_bit(dev, case):
    nq, nc, H, k, seed, chunk, cap = RANDOM_CASES[case][:7]
    q, c, rd, ri = _random_case(dev, case)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, fused=True, seed_rows=seed, chunk=chunk, cand_cap=cap)
    _same(D, I, rd, ri, "fused vs unfused")


# ------------------------------------------------------------------------------------------ 2. integer data: ties at the threshold
@pytest.mark.parametrize("nq,nc,H,k,seed,chunk,cap,sq,sc", INTEGER_CASES)
def test_integer_data_with_ties_matches_the_oracle_bit_for_bit(dev, nq, nc, H, k, seed, chunk, cap, sq, sc):
    """scores are small integers, so many rows tie the running k-th score: a filter that is not strict lists them all (and, for
    the first shape, overflows: the fallback assertion fails), one that is strict against the wrong entry loses rows"""
    q, c = int_emb(sq, nq, H), int_emb(sc, nc, H)
    D, I = _search(dev, q, c, k, id_base=1000, parts=2, fused=True, seed_rows=seed, chunk=chunk, cand_cap=cap)
    rd, ri = orr.search(q, c, k, id_base=1000)
    _same(D, I, rd, ri, "fused vs oracle")


# ------------------------------------------------------------------------------------------ 3. the filter kernel alone
def _filter_case():
    """nq = 130, nc = 300 (ragged tiles both ways), H = 72 (one 64-wide stage + a K tail of 8); even queries hold a full running
    set whose k-th score is the query's 30th best distinct-or-not score (integer data: ties at it), odd queries an open one;
    corpus row 77 holds a binary16 infinity where every query with a zero there scores NaN (query 0 is made one of them)"""
    nq, nc, H, k = 130, 300, 72, 10
    q, c = int_emb(31, nq, H), int_emb(32, nc, H)
    q[0, 5] = 0.0
    c[77, 5] = np.inf
    with np.errstate(invalid="ignore"):
        S = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)      # exact: integers, inf and NaN (0 * inf)
    assert np.isnan(S[0, 77]) and np.isnan(S[:, 77]).sum() > 10 and np.isposinf(S[:, 77]).any()
    thr = np.sort(np.where(np.isfinite(S), S, -1e9), 1)[:, -30].astype(np.float32)
    run_s = thr[:, None] + np.arange(k - 1, -1, -1, dtype=np.float32)[None, :]      # descending, the k-th entry = thr
    run_i = np.tile(np.arange(k, dtype=np.int64), (nq, 1))                          # ids below id0
    run_i[1::2, k - 1] = -1                                                         # odd queries: the set is not full
    with np.errstate(invalid="ignore"):
        expect = ~(S <= thr[:, None])
    expect[1::2] = True
    assert (S == thr[:, None]).sum(1).min() >= 1, "every threshold is tied by at least one row"
    return nq, nc, H, k, q, c, S, run_s, run_i, expect


def _run_filter(dev, cap, guard=64):
    from simxns_amd import _lib as L
    nq, nc, H, k, q, c, S, run_s, run_i, expect = _filter_case()
    id0 = 1000
    tq, tc = torch.from_numpy(q).to(dev).to(torch.float16), torch.from_numpy(c).to(dev).to(torch.float16)
    trs, tri = torch.from_numpy(run_s).to(dev), torch.from_numpy(run_i).to(dev)
    cs = torch.full((nq * cap + guard,), -12345.0, dtype=torch.float32, device=dev)
    ci = torch.full((nq * cap + guard,), -777, dtype=torch.int64, device=dev)
    cnt = torch.zeros(nq + guard, dtype=torch.int32, device=dev)
    L.call("simx_ip_filter_f16", L.stream_ptr(), nq, nc, H, L.ptr(tq), L.ptr(tc), id0, k, L.ptr(trs), L.ptr(tri), L.ptr(cs), L.ptr(ci), cap,
           L.ptr(cnt))
    torch.cuda.synchronize()
    assert (trs.cpu().numpy() == run_s).all() and (tri.cpu().numpy() == run_i).all(), "the filter must not touch the running set"
    cs, ci, cnt = cs.cpu().numpy(), ci.cpu().numpy(), cnt.cpu().numpy()
    assert (cs[nq * cap:] == -12345.0).all() and (ci[nq * cap:] == -777).all() and (cnt[nq:] == 0).all(), "wrote past the arrays"
    return nq, nc, S, expect, id0, cs[:nq * cap].reshape(nq, cap), ci[:nq * cap].reshape(nq, cap), cnt[:nq]


def _entries(scores, ids):
    """{(id, score bits)}, every NaN as one value (its payload is the hardware's)"""
    b = np.where(np.isnan(scores), np.uint32(0x7FC00000), _bits(scores))
    return set(zip(ids.tolist(), b.tolist()))


def test_filter_kernel_lists_exactly_the_survivors(dev):
    nq, nc, S, expect, id0, cs, ci, cnt = _run_filter(dev, cap=512)
    assert (cnt == expect.sum(1)).all(), "cand_count is not the number of survivors"
    for r in range(nq):
        n = cnt[r]
        cols = np.nonzero(expect[r])[0]
        assert _entries(cs[r, :n], ci[r, :n]) == _entries(S[r, cols], cols + id0), "query %d: wrong survivors" % r
        assert (cs[r, n:] == -12345.0).all() and (ci[r, n:] == -777).all(), "query %d: wrote past its count" % r
    assert np.isnan(cs[0, :cnt[0]][ci[0, :cnt[0]] == id0 + 77]).all() and (ci[0, :cnt[0]] == id0 + 77).sum() == 1, "the NaN score is not listed"


def test_filter_kernel_overflow_keeps_the_count_and_the_bounds(dev):
    cap = 16
    nq, nc, S, expect, id0, cs, ci, cnt = _run_filter(dev, cap=cap)
    assert (cnt == expect.sum(1)).all(), "cand_count must keep the true number past cand_cap"
    assert (cnt > cap).any() and (cnt[1::2] == nc).all()
    for r in range(nq):
        n = min(cnt[r], cap)
        cols = np.nonzero(expect[r])[0]
        got = _entries(cs[r, :n], ci[r, :n])
        assert len(got) == n and got <= _entries(S[r, cols], cols + id0), "query %d: an entry that is no survivor of this query" % r
        assert (cs[r, n:] == -12345.0).all() and (ci[r, n:] == -777).all(), "query %d: wrote past its count" % r


def test_filter_kernel_refuses_bad_arguments(dev):
    from simxns_amd import _lib as L
    t = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    i = torch.zeros(4096, dtype=torch.int64, device=dev)
    n = torch.zeros(64, dtype=torch.int32, device=dev)
    good = [4, 8, 16, L.ptr(t), L.ptr(t), 0, 2, L.ptr(f), L.ptr(i), L.ptr(f), L.ptr(i), 8, L.ptr(n)]
    L.call("simx_ip_filter_f16", L.stream_ptr(), *good)
    for pos, bad in ((2, 12), (6, 0), (6, 1025), (11, 0), (5, -1), (5, 2 ** 32), (12, None), (3, None)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(L.SimxError):
            L.call("simx_ip_filter_f16", L.stream_ptr(), *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 4. overflow is counted and repaired
@pytest.mark.parametrize("nq,query_block,blocks", [(3, 8192, 1), (5, 2, 3)])
def test_ascending_scores_overflow_and_fall_back(dev, nq, query_block, blocks):
    """corpus row j = (j, 0, ..): every row beats all rows before it, so every fused chunk lists all its rows (>= 128 > 32)"""
    nc, H, k = 2000, 8, 10
    c = np.zeros((nc, H), np.float32)
    c[:, 0] = np.arange(nc)
    q = np.zeros((nq, H), np.float32)
    q[:, 0] = 1 + np.arange(nq) % 3
    assert (c.astype(np.float16).astype(np.float32) == c).all()
    D, I = _search(dev, q, c, k, fallbacks=blocks, fused=True, seed_rows=128, chunk=512, cand_cap=32, query_block=query_block)
    rd, ri = orr.search(q, c, k)
    _same(D, I, rd, ri, "fallback vs oracle")
    assert (I == np.arange(nc - 1, nc - 1 - k, -1)[None, :]).all()


# ------------------------------------------------------------------------------------------ 5. schedule independence
def test_result_bits_do_not_depend_on_the_schedule(dev):
    nq, nc, H, k, seed, chunk, cap = RANDOM_CASES[0][:7]
    q, c, rd, ri = _random_case(dev, 0)
    base = dict(seed_rows=seed, chunk=chunk, cand_cap=cap)
    settings = ([dict(base, seed_rows=s) for s in (256, 2000, 8192)] + [dict(base, chunk=m) for m in (300, 1000, 65536)] +      # lists <= 88
                [dict(base, cand_cap=n) for n in (256, 300, 4096)] + [dict(base, query_block=b) for b in (7, 64, 8192)])
    for kw in settings:
        D, I = _search(dev, q, c, k, id_base=1000, fused=True, **kw)
        _same(D, I, rd, ri, "fused with %r" % (kw,))


# ------------------------------------------------------------------------------------------ 6. shard merge
def test_two_shards_fold_to_the_global_fused_search(dev):
    from simxns_amd.retrieval import fold_candidates
    nq, nc, H, k, cut = 40, 8000, 256, 200, 3000
    q, c = int_emb(11, nq, H), int_emb(12, nc, H)
    kw = dict(fused=True, seed_rows=1024, chunk=4096, cand_cap=512)          # simulated maxima: 230 / 240 (shards), 237 (global)
    Ds, Is = [], []
    for lo, hi in ((0, cut), (cut, nc)):
        d, i = _search(dev, q, c[lo:hi], k, id_base=lo, **kw)
        Ds.append(torch.from_numpy(d).to(dev)); Is.append(torch.from_numpy(i).to(dev))
    D, I = fold_candidates(torch.cat(Ds, 1).contiguous(), torch.cat(Is, 1).contiguous(), k)
    D1, I1 = _search(dev, q, c, k, **kw)
    _same(D.cpu().numpy(), I.cpu().numpy(), D1, I1, "folded shards vs global")
    rd, ri = orr.search(q, c, k)
    _same(D1, I1, rd, ri, "global vs oracle")


# ------------------------------------------------------------------------------------------ 7. edges
@pytest.mark.parametrize("nq,nc,k,seed", [(5, 100, 10, 128),        # nc <= seed_rows: the seed pass is the whole search
                                          (5, 128, 10, 128),        # ... exactly
                                          (3, 150, 200, 8192),      # k > nc: padded with -inf / -1
                                          (4, 0, 7, 128),           # empty shard
                                          (1, 3000, 10, 128),       # one query
                                          (1, 129, 10, 128)])       # one query, one fused row
def test_edges(dev, nq, nc, k, seed):
    H = 8
    q, c = int_emb(41, nq, H), int_emb(42, nc, H)
    D, I = _search(dev, q, c, k, id_base=7, fused=True, seed_rows=seed, chunk=512, cand_cap=64)     # (1, 3000): lists <= 16 as INTEGER_CASES[1]
    if nc == 0:
        assert (I == -1).all() and np.isneginf(D).all()
        return
    rd, ri = orr.search(q, c, k, id_base=7)
    _same(D, I, rd, ri, "fused vs oracle")
    if k > nc:
        assert (I[:, nc:] == -1).all() and np.isneginf(D[:, nc:]).all()


def test_default_seed_rows_and_cap(dev):
    """the defaults (seed_rows = max(8192, 4 k), cand_cap = 4096) on a shard a little longer than the seed"""
    nq, nc, H, k = 9, 12000, 64, 50
    q, c = f16_emb(51, nq, H), f16_emb(52, nc, H)
    D, I = _search(dev, q, c, k, fused=True)
    rd, ri = _search(dev, q, c, k)
    _same(D, I, rd, ri, "fused defaults vs unfused")


# ------------------------------------------------------------------------------------------ 8. defaults untouched
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_default_index_is_the_unfused_entry_point(dev, storage):
    from simxns_amd import _lib as L
    from simxns_amd.retrieval import FlatIPIndex
    nq, nc, H, k, chunk = 16, 3000, 128, 50, 1024
    q, c = f16_emb(61, nq, H), f16_emb(62, nc, H)
    dt = torch.float16 if storage == "fp16" else torch.float32
    tq, tc = torch.from_numpy(q).to(dev).to(dt), torch.from_numpy(c).to(dev).to(dt)
    index = FlatIPIndex(H, id_base=5, chunk=chunk, storage=storage)
    assert index.fused is False
    index.add(tc)
    D, I = index.search(tq, k)
    assert index.last_search_fallbacks == 0
    n = int(L.load().simx_flat_ip_workspace_bytes(nq, chunk))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    D1 = torch.empty(nq, k, dtype=torch.float32, device=dev)
    I1 = torch.empty(nq, k, dtype=torch.int64, device=dev)
    L.call("simx_flat_ip_search_f16" if storage == "fp16" else "simx_flat_ip_search", L.stream_ptr(), nq, nc, H, L.ptr(tq), L.ptr(tc), 5, k, chunk,
           L.ptr(ws), n, L.ptr(D1), L.ptr(I1))
    torch.cuda.synchronize()
    _same(D.cpu().numpy(), I.cpu().numpy(), D1.cpu().numpy(), I1.cpu().numpy(), "index vs entry point (%s)" % storage)
    rd, ri = orr.search(q, c, k, id_base=5)                    # on binary16-exact rows the float32 chain is the oracle's
    if storage == "fp32":
        _same(D.cpu().numpy(), I.cpu().numpy(), rd, ri, "float32 index vs oracle")
