"""Exhaustive inner-product index on the MI355X -- the role faiss.IndexFlatIP + index_cpu_to_all_gpus(shard=True) play
in the reference's generate job (SimANS/co_training/co_training_generate.py:359-384, 415-421).

One process per GPU holds a contiguous shard of the corpus embeddings in HBM (8.8 M x 768 f32 = 27 GB: the whole
MS-MARCO corpus fits one 288 GB GPU; with W ranks each holds 1/W).  search() = local top-k by the HIP kernels, then --
when a process group is given -- an all_gather of the W x [nq,k] candidates over RCCL and the same top-k kernel as the
merge.  No CPU path: without the HIP library every call raises.

storage="fp16" is faiss's ``useFloat16``: rows and queries are rounded to IEEE binary16 (round to nearest even; values
beyond the binary16 range become +-inf, as in FAISS, and nothing checks for them), the shard takes 2 B per element and the
scores are accumulated in float32 on the matrix cores (ip_scores_f16_kernel).

storage="planes" (opt-in) gives float32-grade scores at matrix-core speed: rows and queries arrive as float32 and are stored as
two binary16 planes, hi = rnd16(x) and lo = rnd16(x - hi) (round to nearest even; the split rule of the fp32 engine, taken on
the device by simx_planes_from), so that |x - hi - lo| <= max(2^-22 |x|, 2^-25) per element.  A score is the float32 MFMA
accumulation of Qhi.Clo + Qlo.Chi + Qhi.Chi -- the lo.lo term is dropped by definition -- in ONE K loop of fixed order (per
64-wide k block: hi.lo, lo.hi, then hi.hi; no split-K, no atomics), so its bits depend on neither the chunk, the query block nor
the position of its row in a tile.  Top-k, tie order (lower id first), padding (-inf, -1) and id_base are as in the other two
modes.  Values beyond the binary16 range are not supported (hi becomes +-inf and nothing checks, as with "fp16"); the embedding
size must be a multiple of 8.  The index holds 4 B per element -- the HBM of "fp32" -- as two separate plane buffers; no float32
copy of the shard is kept.

fused=True (storage="fp16" or "planes", opt-in) searches in one pass: after a short unfused seed pass the score tile is compared
with each query's running k-th entry inside the score kernel (ip_filter_f16_kernel / ip_filter_planes_kernel) and only the
survivors are written, to a per-query candidate list of ``cand_cap`` entries that the top-k kernel folds in.  The result is bit
for bit the unfused one; a query block whose list overflowed (rows in adversarial order) is searched again by the unfused path."""
import ctypes as C

import torch

from . import _lib as L


class FlatIPIndex(object):
    """index = FlatIPIndex(dim); index.add(emb); D, I = index.search(q, k)   (faiss.IndexFlatIP surface)."""

    def __init__(self, dim, id_base=0, chunk=65536, query_block=8192, storage="fp32", fused=False, seed_rows=None, cand_cap=4096):
        """``chunk``: corpus rows scored per pass; ``query_block``: queries per pass -- the score workspace is
        query_block x chunk x 4 B (2 GB by default) whatever the number of queries (the 503 k MS-MARCO train queries in one
        call would otherwise ask for 132 GB).  ``storage``: "fp32" (the default: float32 rows, one fmaf chain per score),
        "fp16" (binary16 rows and queries, float32 scores from the matrix cores; needs dim % 8 == 0) or "planes" (float32 rows
        and queries held as binary16 plane pairs, three-term float32 scores from the matrix cores; needs dim % 8 == 0).
        ``fused``: the one-pass search of the two matrix-core modes (experimental, off by default); its workspace is
        query_block x (seed_rows x 4 + cand_cap x 12) B.
        ``seed_rows``: rows of the unfused first pass, max(8192, 4 k) when None; ``cand_cap``: entries per candidate list.
        ``last_search_fallbacks``: query blocks of the last search() that overflowed a list and were searched again unfused."""
        if storage not in ("fp32", "fp16", "planes"):
            raise ValueError("FlatIPIndex: storage must be 'fp32', 'fp16' or 'planes', not %r" % (storage,))
        if storage != "fp32" and dim % 8 != 0:
            raise ValueError("FlatIPIndex: storage=%r needs an embedding size that is a multiple of 8, not %d" % (storage, dim))
        assert dim % 4 == 0, "embedding size must be a multiple of 4"
        self.d, self.id_base, self.chunk, self.query_block = int(dim), int(id_base), int(chunk), int(query_block)
        self.storage = storage
        self._dtype = torch.float16 if storage == "fp16" else torch.float32
        self._search = {"fp32": "simx_flat_ip_search", "fp16": "simx_flat_ip_search_f16", "planes": "simx_flat_ip_search_planes"}[storage]
        if fused and storage == "fp32":
            raise ValueError("FlatIPIndex: fused=True needs storage='fp16' or 'planes' (the float32 score kernel is bound by its FMA "
                             "rate, not by the score round trip)")
        if int(cand_cap) < 1:
            raise ValueError("FlatIPIndex: cand_cap must be at least 1, not %r" % (cand_cap,))
        if seed_rows is not None and int(seed_rows) < 1:
            raise ValueError("FlatIPIndex: seed_rows must be at least 1, not %r" % (seed_rows,))
        self.fused, self.cand_cap = bool(fused), int(cand_cap)
        self.seed_rows = None if seed_rows is None else int(seed_rows)
        self.last_search_fallbacks = 0
        self._parts, self._emb = [], None                # a stored matrix is a tuple of buffers: (x,), or (hi, lo) for planes

    @property
    def ntotal(self):
        return sum(p[0].shape[0] for p in self._parts) + (0 if self._emb is None else self._emb[0].shape[0])

    def _store(self, x):
        """rows or queries in the index's storage form"""
        x = x.detach().to(self._dtype).contiguous()
        return split_planes(x) if self.storage == "planes" else (x,)

    def _ptrs(self, x, lo=0, n=None):
        """the operand pointers of rows [lo, lo + n) of a stored matrix (None: an empty shard) for the search entry points"""
        if x is None:
            return (None,) * (2 if self.storage == "planes" else 1)
        return tuple(L.ptr(t[lo:] if n is None else t[lo:lo + n]) for t in x)

    def add(self, emb):
        emb = torch.as_tensor(emb)
        if not emb.is_cuda:
            raise L.SimxError("FlatIPIndex.add: embeddings must live on the GPU (there is no CPU path)")
        assert emb.dim() == 2 and emb.shape[1] == self.d
        self._parts.append(self._store(emb))            # planes: split on the device

    def _corpus(self):
        if self._parts:
            parts = ([self._emb] if self._emb is not None else []) + self._parts
            self._emb = tuple(torch.cat(ts, 0) for ts in zip(*parts))      # planes: two buffers
            self._parts = []
        return self._emb

    def search(self, q, k, group=None):
        """-> (scores [nq,k] f32, ids [nq,k] int64), rows sorted by descending score (ties: ascending id); with
        ``group`` every rank passes the SAME queries and receives the global result."""
        q = torch.as_tensor(q)
        if not q.is_cuda:
            raise L.SimxError("FlatIPIndex.search: queries must live on the GPU (there is no CPU path)")
        nq, dev = q.shape[0], q.device
        q = self._store(q)                              # planes: the queries are split once per call
        corpus = self._corpus()
        nc = self.ntotal
        if nc == 0:
            corpus = None
        D = torch.empty(nq, k, dtype=torch.float32, device=dev)
        I = torch.empty(nq, k, dtype=torch.int64, device=dev)
        chunk = max(4, min(self.chunk, max(nc, 4)))
        qb = max(1, min(self.query_block, nq))
        blocks = list(range(0, nq, qb))
        self.last_search_fallbacks = 0
        if self.fused:
            blocks = self._search_fused(q, nq, corpus, nc, k, chunk, qb, blocks, D, I)
            self.last_search_fallbacks = len(blocks)
        if blocks:
            ws_bytes = int(L.load().simx_flat_ip_workspace_bytes(qb, chunk))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for lo in blocks:                               # query blocks reuse ONE workspace
            n = min(qb, nq - lo)
            L.call(self._search, L.stream_ptr(), n, nc, self.d, *self._ptrs(q, lo, n), *self._ptrs(corpus),
                   self.id_base, k, chunk, L.ptr(ws), ws_bytes, L.ptr(D[lo:lo + n]), L.ptr(I[lo:lo + n]))
        if group is None:
            return D, I
        return merge_topk(D, I, k, group)


    def _search_fused(self, q, nq, corpus, nc, k, chunk, qb, blocks, D, I):
        """the one-pass search of every query block; -> the blocks whose candidate lists overflowed (one host read after the loop)"""
        fn = "simx_flat_ip_search_planes_fused" if self.storage == "planes" else "simx_flat_ip_search_f16_fused"
        seed = max(8192, 4 * k) if self.seed_rows is None else self.seed_rows
        seed = max(1, min(seed, nc))                    # no workspace for seed rows the shard does not have
        ws_bytes = int(L.load().simx_flat_ip_fused_workspace_bytes(qb, seed, self.cand_cap))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=D.device)
        overflow = torch.empty(len(blocks), dtype=torch.int32, device=D.device)
        for b, lo in enumerate(blocks):
            n = min(qb, nq - lo)
            L.call(fn, L.stream_ptr(), n, nc, self.d, *self._ptrs(q, lo, n), *self._ptrs(corpus),
                   self.id_base, k, chunk, seed, self.cand_cap, L.ptr(ws), ws_bytes, L.ptr(D[lo:lo + n]), L.ptr(I[lo:lo + n]),
                   L.ptr(overflow[b:b + 1]))
        flags = overflow.cpu().tolist()                 # the one synchronisation of a fused search
        return [lo for lo, f in zip(blocks, flags) if f != 0]


def index_storage(index_float16=False, index_planes=False, index_fused=False):
    """the FlatIPIndex ``storage`` the generate jobs' flags ask for; ValueError (with the text the jobs print) for a combination
    that is refused: both storage flags, or --index_fused with neither"""
    if index_float16 and index_planes:
        raise ValueError("--index_float16 and --index_planes exclude each other: an index has one storage mode")
    if index_fused and not (index_float16 or index_planes):
        raise ValueError("--index_fused needs --index_float16 or --index_planes: the one-pass search exists for the two matrix-core "
                         "index modes only")
    return "fp16" if index_float16 else "planes" if index_planes else "fp32"


def split_planes(x):
    """float32 [n, H] on the GPU (H % 8 == 0) -> (hi, lo): the binary16 plane pair of simx_planes_from, hi = rnd16(x) and
    lo = rnd16(x - hi).  The two planes are the halves of one new [2, n, H] tensor."""
    n, H = x.shape
    pair = torch.empty(2, n, H, dtype=torch.float16, device=x.device)
    if n:
        L.call("simx_planes_from", L.stream_ptr(), L.SIMX_F32, L.SIMX_F16, n, H, L.ptr(x), H, 0, L.ptr(pair), H, n * H)
    return pair[0], pair[1]


def merge_topk(D, I, k, group):
    """all_gather the per-shard results (RCCL) and fold them with the top-k kernel; every rank gets the global top-k."""
    import torch.distributed as dist
    W = dist.get_world_size(group)
    Ds = [torch.empty_like(D) for _ in range(W)]
    Is = [torch.empty_like(I) for _ in range(W)]
    dist.all_gather(Ds, D, group=group)
    dist.all_gather(Is, I, group=group)
    return fold_candidates(torch.cat(Ds, 1).contiguous(), torch.cat(Is, 1).contiguous(), k)


def fold_candidates(cand_scores, cand_ids, k):
    """exact top-k of explicit candidates [nq,m] (ids int64, negative = padding)."""
    nq, m = cand_scores.shape
    D = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=cand_scores.device)
    I = torch.full((nq, k), -1, dtype=torch.int64, device=cand_scores.device)
    L.call("simx_topk_update", L.stream_ptr(), nq, m, L.ptr(cand_scores), m, L.ptr(cand_ids), m, 0, k, L.ptr(D), L.ptr(I))
    return D, I
