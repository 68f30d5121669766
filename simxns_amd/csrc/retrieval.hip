// Generate job: exhaustive inner-product search over a corpus shard resident in HBM -- the role of
// faiss.IndexFlatIP + index_cpu_to_all_gpus in SimANS/co_training/co_training_generate.py:359-384, 415-421.
//
//   ip_scores_kernel   S[nq, chunk] = Q . C^T in float32, ONE fused-multiply-add chain per score in ascending h
//                      (bit-reproducible: oracle/topk_ref.c restates exactly this), 128x128x16 register-tiled
//                      VALU kernel (the f32 MFMA has the same peak as packed f32 FMA on gfx950 and no defined
//                      accumulation order).  Bound: f32 FMA, 2*nq*nc*H FLOP.
//   ip_scores_f16_kernel  the same contraction for the float16 storage mode (faiss useFloat16): both operands binary16, products
//                      exact in float32, float32 accumulation by v_mfma_f32_16x16x32_f16 in ONE K loop of fixed order per
//                      score (no split-K, no atomics), so a score depends on neither the chunk, the query block nor the
//                      position of its row in a tile.  128x128x64 tiles, LDS-DMA staging into the swizzled image of the
//                      NT GEMMs, K tail zero-filled in LDS.  Bounds: 16-bit MFMA rate and, for a whole search, the 8 B
//                      of HBM traffic per score of the write-then-top-k design.
//   ip_scores_planes_kernel / ip_filter_planes_kernel  the plane-pair storage mode: every float32 row and query is held as two binary16
//                      planes, hi = rnd16(x), lo = rnd16(x - hi) (the plane_split2 rule of common.h, taken by simx_planes_from), and a
//                      score is the float32 MFMA accumulation of Qhi.Clo + Qlo.Chi + Qhi.Chi (lo.lo dropped by definition): 22
//                      significand bits per operand element on the 16-bit matrix cores.  The loop is iph_main_loop<true>: the same
//                      staging, LDS image, fragment reads and K order as the binary16 kernels, with four operand tiles per stage and
//                      three products per 64-wide k block in the fixed order hi.lo, lo.hi, hi.hi; the epilogues are the ones of the
//                      binary16 kernels.  Tile choice: BK stays 64, so the two stages take 128 KB of LDS and ONE workgroup runs per CU.
//                      A k block is 96 MFMAs per wave against 64 KB of LDS-DMA, so the next stage lands well inside the matrix
//                      work of the current one and a second workgroup has little latency left to hide; BK = 32 would keep two
//                      workgroups but needs a second LDS image (64-B rows, another swizzle) and a barrier plus a fragment-read
//                      restart every 32-deep step, which is the slower form of this loop.  Bounds: 3 x the 16-bit MFMA work of the
//                      binary16 kernels for 2 x their operand bytes.
//   ip_filter_f16_kernel  the same main loop (iph_main_loop: ONE copy, so a score has the same bits in both kernels) with a
//                      filter epilogue instead of the store: each score is compared, still in the accumulators, with the running
//                      k-th entry of its query (run_scores / run_ids [q*k + k-1]; id < 0 = the set is not full and everything
//                      survives); it survives if !(score <= thr), which keeps NaN and is strict on ties.  A survivor takes a slot
//                      with a device-scope atomicAdd on cand_count[q] and, if slot < cand_cap, writes (score, id0 + column) to the
//                      query's candidate list; the count keeps the true number, so an overflow is visible.
//                      PRECONDITION of the strict test: every row scored here has a LARGER id than every entry of the running set
//                      (inside one search over one shard: the rows of a later chunk).  A row that ties the k-th score then loses
//                      on the id rule (ties: ascending id) exactly as in topk_stream_kernel.  The filter may pass a score the fold
//                      rejects; it never drops one whose key exceeds the running k-th key (a threshold of -0.0 is lowered to
//                      -FLT_MIN, since +0.0 <= -0.0 but key(+0.0) > key(-0.0)).
//   topk_stream_kernel per query: streaming exact top-k over [running best (k) U new candidates] with 64-bit
//                      composite keys (orderable score << 32 | ~id): candidates below the running k-th key are
//                      dropped while scanning, survivors are collected in LDS and folded in by a bitonic sort of
//                      4096 keys whenever the buffer could overflow.  Ties: lower id first.  HBM-bound: reads the
//                      score row once (4 B per candidate).  With a per-query count (the fold of the filter kernels'
//                      lists) the rows of query q are its first min(cand_count[q], cand_cap) list entries, the sort is sized
//                      to the next power of two >= k + that number, a count above cand_cap adds 1 to the overflow word and
//                      the count is reset to 0 for the next chunk.
#include <float.h>
#include <math.h>
#include "common.h"
#include "p3.h"
#include "prof.h"

#define IP_BM 128
#define IP_BN 128
#define IP_BK 16

__global__ __launch_bounds__(256) void ip_scores_kernel(int nq, int nc, int H, const float* __restrict__ Q,
                                                        const float* __restrict__ Cp, float* __restrict__ S, long ldS) {
  __shared__ __attribute__((aligned(16))) float As[IP_BK][IP_BM + 4];
  __shared__ __attribute__((aligned(16))) float Bs[IP_BK][IP_BN + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * IP_BM, n0 = blockIdx.x * IP_BN;
  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < H; k0 += IP_BK) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int idx = tid + e * 256, row = idx >> 2, kq = (idx & 3) * 4;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (k0 + kq < H) {
        if (m0 + row < nq) a = *reinterpret_cast<const float4*>(Q + (long)(m0 + row) * H + k0 + kq);
        if (n0 + row < nc) b = *reinterpret_cast<const float4*>(Cp + (long)(n0 + row) * H + k0 + kq);
      }
      As[kq + 0][row] = a.x; As[kq + 1][row] = a.y; As[kq + 2][row] = a.z; As[kq + 3][row] = a.w;
      Bs[kq + 0][row] = b.x; Bs[kq + 1][row] = b.y; Bs[kq + 2][row] = b.z; Bs[kq + 3][row] = b.w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < IP_BK; ++kk) {
      const float4 a0 = *reinterpret_cast<const float4*>(&As[kk][ty * 4]), a1 = *reinterpret_cast<const float4*>(&As[kk][64 + ty * 4]);
      const float4 b0 = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]), b1 = *reinterpret_cast<const float4*>(&Bs[kk][64 + tx * 4]);
      const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + (i - 4));
    if (m >= nq) continue;
#pragma unroll
    for (int jh = 0; jh < 2; ++jh) {
      const int n = n0 + jh * 64 + tx * 4;
      float* dst = S + (long)m * ldS + n;
      if (n + 4 <= nc && (ldS & 3) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[i][jh * 4 + 0], acc[i][jh * 4 + 1], acc[i][jh * 4 + 2], acc[i][jh * 4 + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n + j < nc) dst[j] = acc[i][jh * 4 + j];
      }
    }
  }
}

// ---- float16 storage: scores on the matrix cores ----------------------------------------------------------------------
#define IPH_BM 128
#define IPH_BN 128
#define IPH_BK 64
#define IPH_TILE (128 * 64 * 2)            // one operand tile; a stage = Q tile + C tile

// stage rows [row0, row0 + 128) x k [k0, k0 + 64) of G [nrows, H] (binary16, K contiguous).  LDS image as in the NT GEMMs:
// row r at r * 128 B, the 16-B chunk c of the row at chunk position c ^ ((r >> 1) & 7).  Rows past the end re-read the last
// row (their scores are never stored).  A full stage goes by LDS-DMA; the ragged last stage (H % 64 != 0; H % 8 == 0, so a
// chunk is inside the row or wholly outside it) through registers, with zeros for the chunks at k >= H: no byte past a row
// is ever read.
__device__ __forceinline__ void iph_stage_tile(const f16_t* __restrict__ G, int H, int row0, int nrows, int k0, char* tile,
                                               int wave, int lane) {
  const bool full = k0 + IPH_BK <= H;          // uniform
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = wave * 4 + j;                // wave-instruction index: 8 rows each
    const int r = i * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    int gr = row0 + r;
    gr = gr < nrows ? gr : nrows - 1;
    const f16_t* src = G + (long)gr * H + k0 + c * 8;
    if (full) {
      glds16(src, tile + i * 1024);
    } else {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k0 + c * 8 < H) v = *reinterpret_cast<const uint4*>(src);
      *reinterpret_cast<uint4*>(tile + i * 1024 + lane * 16) = v;
    }
  }
}

// one stage = the operand tiles of one k block: [Q][C] for binary16 operands, [Q hi][C hi][Q lo][C lo] for plane pairs
template <bool PLANES>
__device__ __forceinline__ void iph_stage(int nq, int nc, int H, const f16_t* Q, const f16_t* Ql, const f16_t* Cp, const f16_t* Cl, int m0,
                                          int n0, int k0, char* st, int wave, int lane) {
  iph_stage_tile(Q, H, m0, nq, k0, st, wave, lane);
  iph_stage_tile(Cp, H, n0, nc, k0, st + IPH_TILE, wave, lane);
  if constexpr (PLANES) {
    iph_stage_tile(Ql, H, m0, nq, k0, st + 2 * IPH_TILE, wave, lane);
    iph_stage_tile(Cl, H, n0, nc, k0, st + 3 * IPH_TILE, wave, lane);
  }
}

// the ONE main loop of the matrix-core score kernels: acc[i][j] = the 16 x 16 tiles (query rows wr * 64 + i * 16 .., passages
// wc * 64 + j * 16 ..) of the 128 x 128 tile at (m0, n0), accumulated over all of H in ascending k.
//   PLANES == false: binary16 operands Q, Cp (Ql, Cl unused), one product per k block.
//   PLANES == true : plane pairs (Q, Ql) and (Cp, Cl), three products per k block into the same accumulators, in the fixed order
//                    hi.lo, lo.hi, hi.hi (corrections first, as gemm_xp.hip; lo.lo is dropped by definition).
template <bool PLANES>
__device__ __forceinline__ void iph_main_loop(int nq, int nc, int H, const f16_t* Q, const f16_t* Ql, const f16_t* Cp, const f16_t* Cl,
                                              int m0, int n0, char* smem, int wave, int lane, f32x4 (&acc)[4][4]) {
  constexpr int STAGE = (PLANES ? 4 : 2) * IPH_TILE;
  constexpr int TERMS = PLANES ? 3 : 1;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nt = (H + IPH_BK - 1) / IPH_BK;
  iph_stage<PLANES>(nq, nc, H, Q, Ql, Cp, Cl, m0, n0, 0, smem, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int fr = lane & 15, fg = lane >> 4;
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const char* st = smem + cur * STAGE;
    if (t + 1 < nt) iph_stage<PLANES>(nq, nc, H, Q, Ql, Cp, Cl, m0, n0, (t + 1) * IPH_BK, smem + (cur ^ 1) * STAGE, wave, lane);
#pragma unroll
    for (int term = 0; term < TERMS; ++term) {   // plane pairs: Q hi . C lo, Q lo . C hi, Q hi . C hi
      const char* sa = st + (PLANES && term == 1 ? 2 * IPH_TILE : 0);
      const char* sb = st + IPH_TILE + (PLANES && term == 0 ? 2 * IPH_TILE : 0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {           // ascending k: the one accumulation order of a score
        bf16x8 af[4], bfr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ra = wr * 64 + i * 16 + fr;
          af[i] = *reinterpret_cast<const bf16x8*>(sa + ra * 128 + (((ks * 4 + fg) ^ ((ra >> 1) & 7)) << 4));
          const int rb = wc * 64 + i * 16 + fr;
          bfr[i] = *reinterpret_cast<const bf16x8*>(sb + rb * 128 + (((ks * 4 + fg) ^ ((rb >> 1) & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = H16<f16_t>::mfma(bfr[j], af[i], acc[i][j]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
}

// the tile a workgroup scores.  Queries fastest: the workgroups of one XCD walk all query tiles of a few corpus tiles, so a corpus
// row leaves HBM once
struct IphTile { int m0, n0, lane, wave; };
__device__ __forceinline__ IphTile iph_tile(int tiles_m, int nwg) {
  IphTile t;
  t.lane = threadIdx.x & 63;
  t.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = xcd_remap(blockIdx.x, nwg);
  t.m0 = (tile % tiles_m) * IPH_BM;
  t.n0 = (tile / tiles_m) * IPH_BN;
  return t;
}

// store epilogue: lane holds query m = .. + fr, passages n = .. + fg * 4 .. + 3 of each 16 x 16 tile
__device__ __forceinline__ void iph_store(const IphTile& t, int nq, int nc, const f32x4 (&acc)[4][4], float* __restrict__ S, long ldS) {
  const int wr = t.wave >> 1, wc = t.wave & 1, fr = t.lane & 15, fg = t.lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = t.m0 + wr * 64 + i * 16 + fr;
    if (m >= nq) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = t.n0 + wc * 64 + j * 16 + fg * 4;
      float* dst = S + (long)m * ldS + n;
      if (n + 4 <= nc && (ldS & 3) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < nc) dst[e] = acc[i][j][e];
      }
    }
  }
}

// filter epilogue (see the header of this file for the rule and its precondition).  Survivors are rare once the running set is
// warm -- about k * nc / rows_seen per query and chunk -- so a 16 x 16 tile is first tested with one wave-wide ballot.
struct IphFilter {
  float thr[4];
  bool open[4];                                  // the row takes every score: its set is not full
  bool live[4];                                  // the row exists
};
// the running k-th entry of the lane's four query rows, loaded ahead of the main loop
__device__ __forceinline__ IphFilter iph_filter_load(const IphTile& t, int nq, int k, const float* __restrict__ run_s,
                                                     const long long* __restrict__ run_i) {
  const int wr = t.wave >> 1, fr = t.lane & 15;
  IphFilter f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = t.m0 + wr * 64 + i * 16 + fr;
    f.live[i] = m < nq;
    f.thr[i] = 0.f;
    f.open[i] = false;
    if (f.live[i]) {
      const long at = (long)m * k + (k - 1);
      f.open[i] = run_i[at] < 0;
      const float v = run_s[at];
      f.thr[i] = __float_as_uint(v) == 0x80000000u ? -FLT_MIN : v;
    }
  }
  return f;
}
__device__ __forceinline__ void iph_filter(const IphTile& t, const IphFilter& f, int nc, const f32x4 (&acc)[4][4], long long id0,
                                           float* __restrict__ cand_s, long long* __restrict__ cand_i, int cand_cap,
                                           int* __restrict__ cand_count) {
  const int wr = t.wave >> 1, wc = t.wave & 1, fr = t.lane & 15, fg = t.lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = t.m0 + wr * 64 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = t.n0 + wc * 64 + j * 16 + fg * 4;
      bool pass[4];
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pass[e] = f.live[i] && n + e < nc && (f.open[i] || !(acc[i][j][e] <= f.thr[i]));
        any = any || pass[e];
      }
      if (__ballot(any) == 0ull) continue;       // wave-uniform: no survivor in this 16 x 16 tile
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!pass[e]) continue;
        const int slot = atomicAdd(cand_count + m, 1);          // device scope: one query's workgroups sit on different XCDs
        if (slot < cand_cap) {
          cand_s[(long)m * cand_cap + slot] = acc[i][j][e];
          cand_i[(long)m * cand_cap + slot] = id0 + n + e;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256, 2) void ip_scores_f16_kernel(int nq, int nc, int H, const f16_t* __restrict__ Q,
                                                               const f16_t* __restrict__ Cp, float* __restrict__ S, long ldS,
                                                               int tiles_m, int nwg) {
  __shared__ __attribute__((aligned(16))) char smem[4 * IPH_TILE];
  const IphTile t = iph_tile(tiles_m, nwg);
  f32x4 acc[4][4];
  iph_main_loop<false>(nq, nc, H, Q, nullptr, Cp, nullptr, t.m0, t.n0, smem, t.wave, t.lane, acc);
  iph_store(t, nq, nc, acc, S, ldS);
}

__global__ __launch_bounds__(256, 2) void ip_filter_f16_kernel(int nq, int nc, int H, const f16_t* __restrict__ Q,
                                                               const f16_t* __restrict__ Cp, long long id0, int k,
                                                               const float* __restrict__ run_s, const long long* __restrict__ run_i,
                                                               float* __restrict__ cand_s, long long* __restrict__ cand_i, int cand_cap,
                                                               int* __restrict__ cand_count, int tiles_m, int nwg) {
  __shared__ __attribute__((aligned(16))) char smem[4 * IPH_TILE];
  const IphTile t = iph_tile(tiles_m, nwg);
  const IphFilter f = iph_filter_load(t, nq, k, run_s, run_i);
  f32x4 acc[4][4];
  iph_main_loop<false>(nq, nc, H, Q, nullptr, Cp, nullptr, t.m0, t.n0, smem, t.wave, t.lane, acc);
  iph_filter(t, f, nc, acc, id0, cand_s, cand_i, cand_cap, cand_count);
}

// plane-pair storage: the same two kernels on the three-term loop.  Two stages of four tiles are 128 KB of (dynamic) LDS: one
// workgroup per CU.
#define IPP_LDS (8 * IPH_TILE)
__global__ __launch_bounds__(256, 1) void ip_scores_planes_kernel(int nq, int nc, int H, const f16_t* __restrict__ Qh,
                                                                  const f16_t* __restrict__ Ql, const f16_t* __restrict__ Ch,
                                                                  const f16_t* __restrict__ Cl, float* __restrict__ S, long ldS,
                                                                  int tiles_m, int nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const IphTile t = iph_tile(tiles_m, nwg);
  f32x4 acc[4][4];
  iph_main_loop<true>(nq, nc, H, Qh, Ql, Ch, Cl, t.m0, t.n0, smem, t.wave, t.lane, acc);
  iph_store(t, nq, nc, acc, S, ldS);
}

__global__ __launch_bounds__(256, 1) void ip_filter_planes_kernel(int nq, int nc, int H, const f16_t* __restrict__ Qh,
                                                                  const f16_t* __restrict__ Ql, const f16_t* __restrict__ Ch,
                                                                  const f16_t* __restrict__ Cl, long long id0, int k,
                                                                  const float* __restrict__ run_s, const long long* __restrict__ run_i,
                                                                  float* __restrict__ cand_s, long long* __restrict__ cand_i, int cand_cap,
                                                                  int* __restrict__ cand_count, int tiles_m, int nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const IphTile t = iph_tile(tiles_m, nwg);
  const IphFilter f = iph_filter_load(t, nq, k, run_s, run_i);
  f32x4 acc[4][4];
  iph_main_loop<true>(nq, nc, H, Qh, Ql, Ch, Cl, t.m0, t.n0, smem, t.wave, t.lane, acc);
  iph_filter(t, f, nc, acc, id0, cand_s, cand_i, cand_cap, cand_count);
}

// ---- top-k ------------------------------------------------------------------------------------------------------
#define TK_N 4096            // keys sorted per flush (32 KB of LDS)
#define TK_KMAX 1024
#define TK_SEG 2048          // candidates scanned between overflow checks

__device__ __forceinline__ uint64_t tk_key(float s, long long id) {
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
}
__device__ __forceinline__ void tk_unkey(uint64_t key, float* s, long long* id) {
  if (key == 0) { *s = -INFINITY; *id = -1; return; }
  uint32_t u = (uint32_t)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  *s = __uint_as_float(u);
  *id = (long long)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu));
}

// descending bitonic sort of arr[0..n), n a power of two <= TK_N (256 threads)
__device__ void tk_sort(uint64_t* arr, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // lower index of the pair
        const int p = i | j;
        const bool desc = (i & k) == 0;
        const uint64_t x = arr[i], y = arr[p];
        if ((x < y) == desc) { arr[i] = y; arr[p] = x; }
      }
      __syncthreads();
    }
  }
}

// cand_count == nullptr: m candidates per query, scores[q * ld + j] with ids[q * ld_ids + j] or id_base + j.
// cand_count != nullptr: the lists of the filter kernels (ids explicit, ld = ld_ids = cand_cap = m): query q has
// min(cand_count[q], m) entries; a count above m adds 1 to *overflow; the count is reset to 0.
__global__ __launch_bounds__(256) void topk_stream_kernel(int m, const float* __restrict__ scores, long ld,
                                                          const long long* __restrict__ ids, long ld_ids, long long id_base,
                                                          int k, float* __restrict__ run_s, long long* __restrict__ run_i,
                                                          int* __restrict__ cand_count, int* __restrict__ overflow) {
  __shared__ uint64_t arr[TK_N];
  __shared__ int cnt, listed;
  const int q = blockIdx.x, tid = threadIdx.x;
  int n = TK_N;                                    // keys sorted per flush
  if (cand_count) {
    if (tid == 0) listed = cand_count[q];
    __syncthreads();
    const int c = listed;
    if (c == 0) return;                            // uniform: nothing survived, the running set stands
    if (tid == 0) {
      cand_count[q] = 0;
      if (c > m) atomicAdd(overflow, 1);
    }
    m = min(c, m);
    while ((n >> 1) >= k + m) n >>= 1;             // the next power of two >= k + m (TK_N when the list needs flushes)
  }
  const float* row = scores + (long)q * ld;
  const long long* idr = ids ? ids + (long)q * ld_ids : nullptr;
  for (int t = tid; t < n; t += 256) {
    uint64_t key = 0;
    if (t < k) { const long long id = run_i[(long)q * k + t]; if (id >= 0) key = tk_key(run_s[(long)q * k + t], id); }
    arr[t] = key;
  }
  if (tid == 0) cnt = 0;
  __syncthreads();
  const int cap = n - k;
  for (int s0 = 0; s0 < m; s0 += TK_SEG) {
    const int s1 = min(m, s0 + TK_SEG);
    if (cnt + (s1 - s0) > cap) {                   // uniform: fold the buffer into the best-k first
      __syncthreads();
      tk_sort(arr, n);
      for (int t = k + tid; t < n; t += 256) arr[t] = 0;
      if (tid == 0) cnt = 0;
      __syncthreads();
    }
    const uint64_t tau = arr[k - 1];               // running k-th key (0 while fewer than k are known)
    __syncthreads();
    for (int j = s0 + tid; j < s1; j += 256) {
      const long long id = idr ? idr[j] : id_base + j;
      if (id < 0) continue;
      const uint64_t key = tk_key(row[j], id);
      if (key > tau) arr[k + atomicAdd(&cnt, 1)] = key;
    }
    __syncthreads();
  }
  tk_sort(arr, n);
  for (int t = tid; t < k; t += 256) {
    float s; long long id;
    tk_unkey(arr[t], &s, &id);
    run_s[(long)q * k + t] = s;
    run_i[(long)q * k + t] = id;
  }
}

extern "C" int simx_ip_scores(simx_stream_t stream, int nq, int nc, int H, const float* q, const float* c, float* scores, long ld) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_PROF(SIMX_K_TOPK, s, 2.0 * nq * nc * H);
  SIMX_REQUIRE(nq > 0 && nc > 0 && H > 0 && H % 4 == 0 && ld >= nc, SIMX_ERR_BAD_SHAPE, "ip_scores: bad shape nq=%d nc=%d H=%d ld=%ld", nq, nc, H, ld);
  SIMX_REQUIRE(simx_al16(q) && simx_al16(c) && simx_al16(scores), SIMX_ERR_BAD_SHAPE, "ip_scores: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(ip_scores_kernel, dim3(cdiv(nc, IP_BN), cdiv(nq, IP_BM)), dim3(256), 0, s, nq, nc, H, q, c, scores, ld);
  SIMX_CHECK_LAUNCH("ip_scores");
  return SIMX_OK;
}

// operands of the matrix-core kernels: binary16 matrices (lo == nullptr) or binary16 plane pairs (hi, lo)
struct IphOperand { const f16_t *hi, *lo; };
static bool iph_ok(const IphOperand& x, bool planes) { return x.hi && simx_al16(x.hi) && (!planes || (x.lo && simx_al16(x.lo))); }
static IphOperand iph_rows(const IphOperand& x, long row0, int H) { return IphOperand{x.hi + row0 * H, x.lo ? x.lo + row0 * H : nullptr}; }

// the dynamic-LDS limit of the plane-pair kernels (more than 64 KB), set once per device; false: it could not be set
static bool ip_planes_device() {
  static SimxLdsAttrs st;
  static const SimxLdsAttr lds[] = {simx_lds(ip_scores_planes_kernel, IPP_LDS), simx_lds(ip_filter_planes_kernel, IPP_LDS)};
  return simx_set_lds_attrs(st, lds, sizeof(lds) / sizeof(lds[0]));
}

// the score launcher of both matrix-core modes (`what` names the entry point in messages)
static int ip_scores_h16(const char* what, bool planes, simx_stream_t stream, int nq, int nc, int H, IphOperand q, IphOperand c, float* scores,
                         long ld) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_PROF(SIMX_K_TOPK, s, (planes ? 6.0 : 2.0) * nq * nc * H);
  SIMX_REQUIRE(nq > 0 && nc > 0 && H > 0 && H % 8 == 0 && ld >= nc, SIMX_ERR_BAD_SHAPE, "%s: bad shape nq=%d nc=%d H=%d ld=%ld", what, nq, nc, H, ld);
  SIMX_REQUIRE(iph_ok(q, planes) && iph_ok(c, planes) && scores && simx_al16(scores), SIMX_ERR_BAD_SHAPE,
               "%s: pointers must be non-NULL and 16-byte aligned", what);
  const int tiles_m = cdiv(nq, IPH_BM), tiles_n = cdiv(nc, IPH_BN);
  SIMX_REQUIRE((long)tiles_m * tiles_n <= 0x7FFFFFFFl, SIMX_ERR_BAD_SHAPE, "%s: too many tiles (nq=%d nc=%d)", what, nq, nc);
  const int nwg = tiles_m * tiles_n;
  SIMX_REQUIRE(!planes || ip_planes_device(), SIMX_ERR_HIP, "%s: the LDS limit of the plane kernels could not be set", what);
  if (planes) hipLaunchKernelGGL(ip_scores_planes_kernel, dim3(nwg), dim3(256), IPP_LDS, s, nq, nc, H, q.hi, q.lo, c.hi, c.lo, scores, ld, tiles_m, nwg);
  else hipLaunchKernelGGL(ip_scores_f16_kernel, dim3(nwg), dim3(256), 0, s, nq, nc, H, q.hi, c.hi, scores, ld, tiles_m, nwg);
  SIMX_CHECK_LAUNCH(what);
  return SIMX_OK;
}

// the filter launcher of both matrix-core modes
static int ip_filter_h16(const char* what, bool planes, simx_stream_t stream, int nq, int nc, int H, IphOperand q, IphOperand c, int64_t id0, int k,
                         const float* run_scores, const int64_t* run_ids, float* cand_scores, int64_t* cand_ids, int cand_cap, int* cand_count) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_PROF(SIMX_K_TOPK, s, (planes ? 6.0 : 2.0) * nq * nc * H);
  SIMX_REQUIRE(nq > 0 && nc > 0 && H > 0 && H % 8 == 0, SIMX_ERR_BAD_SHAPE, "%s: bad shape nq=%d nc=%d H=%d", what, nq, nc, H);
  SIMX_REQUIRE(k > 0 && k <= TK_KMAX && cand_cap > 0, SIMX_ERR_BAD_SHAPE, "%s: need 0 < k=%d <= %d and cand_cap=%d > 0", what, k, TK_KMAX, cand_cap);
  SIMX_REQUIRE(iph_ok(q, planes) && iph_ok(c, planes), SIMX_ERR_BAD_SHAPE, "%s: the operands must be non-NULL and 16-byte aligned", what);
  SIMX_REQUIRE(run_scores && run_ids && cand_scores && cand_ids && cand_count, SIMX_ERR_BAD_SHAPE, "%s: NULL argument", what);
  SIMX_REQUIRE(id0 >= 0 && id0 + nc < 0xFFFFFFFFll, SIMX_ERR_BAD_SHAPE, "%s: ids must fit 32 bits", what);
  const int tiles_m = cdiv(nq, IPH_BM), tiles_n = cdiv(nc, IPH_BN);
  SIMX_REQUIRE((long)tiles_m * tiles_n <= 0x7FFFFFFFl, SIMX_ERR_BAD_SHAPE, "%s: too many tiles (nq=%d nc=%d)", what, nq, nc);
  const int nwg = tiles_m * tiles_n;
  SIMX_REQUIRE(!planes || ip_planes_device(), SIMX_ERR_HIP, "%s: the LDS limit of the plane kernels could not be set", what);
  if (planes)
    hipLaunchKernelGGL(ip_filter_planes_kernel, dim3(nwg), dim3(256), IPP_LDS, s, nq, nc, H, q.hi, q.lo, c.hi, c.lo, (long long)id0, k, run_scores,
                       (const long long*)run_ids, cand_scores, (long long*)cand_ids, cand_cap, cand_count, tiles_m, nwg);
  else
    hipLaunchKernelGGL(ip_filter_f16_kernel, dim3(nwg), dim3(256), 0, s, nq, nc, H, q.hi, c.hi, (long long)id0, k, run_scores,
                       (const long long*)run_ids, cand_scores, (long long*)cand_ids, cand_cap, cand_count, tiles_m, nwg);
  SIMX_CHECK_LAUNCH(what);
  return SIMX_OK;
}

extern "C" int simx_ip_scores_f16(simx_stream_t stream, int nq, int nc, int H, const void* q16, const void* c16, float* scores, long ld) {
  return ip_scores_h16("ip_scores_f16", false, stream, nq, nc, H, IphOperand{(const f16_t*)q16, nullptr}, IphOperand{(const f16_t*)c16, nullptr}, scores, ld);
}

extern "C" int simx_ip_scores_planes(simx_stream_t stream, int nq, int nc, int H, const void* q_hi, const void* q_lo, const void* c_hi, const void* c_lo,
                                     float* scores, long ld) {
  return ip_scores_h16("ip_scores_planes", true, stream, nq, nc, H, IphOperand{(const f16_t*)q_hi, (const f16_t*)q_lo},
                       IphOperand{(const f16_t*)c_hi, (const f16_t*)c_lo}, scores, ld);
}

extern "C" int simx_ip_filter_f16(simx_stream_t stream, int nq, int nc, int H, const void* q16, const void* c16, int64_t id0, int k,
                                  const float* run_scores, const int64_t* run_ids, float* cand_scores, int64_t* cand_ids, int cand_cap,
                                  int* cand_count) {
  return ip_filter_h16("ip_filter_f16", false, stream, nq, nc, H, IphOperand{(const f16_t*)q16, nullptr}, IphOperand{(const f16_t*)c16, nullptr}, id0, k,
                       run_scores, run_ids, cand_scores, cand_ids, cand_cap, cand_count);
}

extern "C" int simx_ip_filter_planes(simx_stream_t stream, int nq, int nc, int H, const void* q_hi, const void* q_lo, const void* c_hi, const void* c_lo,
                                     int64_t id0, int k, const float* run_scores, const int64_t* run_ids, float* cand_scores, int64_t* cand_ids,
                                     int cand_cap, int* cand_count) {
  return ip_filter_h16("ip_filter_planes", true, stream, nq, nc, H, IphOperand{(const f16_t*)q_hi, (const f16_t*)q_lo},
                       IphOperand{(const f16_t*)c_hi, (const f16_t*)c_lo}, id0, k, run_scores, run_ids, cand_scores, cand_ids, cand_cap, cand_count);
}

extern "C" int simx_topk_update(simx_stream_t stream, int nq, int m, const float* scores, long ld, const int64_t* ids, long ld_ids,
                                int64_t id_base, int k, float* run_scores, int64_t* run_ids) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(nq > 0 && m >= 0 && k > 0 && k <= TK_KMAX, SIMX_ERR_BAD_SHAPE, "topk_update: need 0 < k=%d <= %d", k, TK_KMAX);
  SIMX_REQUIRE(scores && run_scores && run_ids && ld >= m, SIMX_ERR_BAD_SHAPE, "topk_update: NULL argument / ld < m");
  SIMX_REQUIRE(ids != nullptr || (id_base >= 0 && id_base + m < 0xFFFFFFFFll), SIMX_ERR_BAD_SHAPE, "topk_update: ids must fit 32 bits");
  hipLaunchKernelGGL(topk_stream_kernel, dim3(nq), dim3(256), 0, s, m, scores, ld, (const long long*)ids, ld_ids, (long long)id_base, k,
                     run_scores, (long long*)run_ids, (int*)nullptr, (int*)nullptr);
  SIMX_CHECK_LAUNCH("topk_update");
  return SIMX_OK;
}

extern "C" int simx_topk_fold_lists(simx_stream_t stream, int nq, const float* cand_scores, const int64_t* cand_ids, int cand_cap,
                                    int* cand_count, int k, float* run_scores, int64_t* run_ids, int* overflow) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(nq > 0 && cand_cap > 0 && k > 0 && k <= TK_KMAX, SIMX_ERR_BAD_SHAPE, "topk_fold_lists: need nq=%d > 0, cand_cap=%d > 0, 0 < k=%d <= %d", nq,
               cand_cap, k, TK_KMAX);
  SIMX_REQUIRE(cand_scores && cand_ids && cand_count && run_scores && run_ids && overflow, SIMX_ERR_BAD_SHAPE, "topk_fold_lists: NULL argument");
  hipLaunchKernelGGL(topk_stream_kernel, dim3(nq), dim3(256), 0, s, cand_cap, cand_scores, (long)cand_cap, (const long long*)cand_ids, (long)cand_cap,
                     0ll, k, run_scores, (long long*)run_ids, cand_count, overflow);
  SIMX_CHECK_LAUNCH("topk_fold_lists");
  return SIMX_OK;
}

__global__ void topk_init_kernel(long n, float* s, long long* i) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) { s[t] = -INFINITY; i[t] = -1; }
}

extern "C" size_t simx_flat_ip_workspace_bytes(int nq, int chunk) { return (size_t)nq * (size_t)((chunk + 3) & ~3) * sizeof(float); }

// index.search over a shard in one of the three storage modes: the chunk walk is the same, the score kernel differs
enum IpMode { IP_F32, IP_F16, IP_PLANES };
static int flat_ip_search(const char* what, IpMode mode, simx_stream_t stream, int nq, long nc, int H, const void* q, const void* q_lo,
                          const void* corpus, const void* corpus_lo, int64_t id_base, int k, int chunk, void* workspace, size_t workspace_bytes,
                          float* out_scores, int64_t* out_ids) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(nq > 0 && nc >= 0 && chunk > 0, SIMX_ERR_BAD_SHAPE, "%s: bad shape", what);
  SIMX_REQUIRE(workspace_bytes >= simx_flat_ip_workspace_bytes(nq, chunk), SIMX_ERR_WORKSPACE, "%s: workspace too small", what);
  const long ld = (chunk + 3) & ~3;
  const IphOperand q16{(const f16_t*)q, (const f16_t*)q_lo}, c16{(const f16_t*)corpus, (const f16_t*)corpus_lo};
  hipLaunchKernelGGL(topk_init_kernel, dim3(cdiv((int)((long)nq * k), 256)), dim3(256), 0, s, (long)nq * k, out_scores, (long long*)out_ids);
  SIMX_CHECK_LAUNCH("topk_init");
  for (long c0 = 0; c0 < nc; c0 += chunk) {
    const int m = (int)((nc - c0) < chunk ? (nc - c0) : chunk);
    int rc = mode == IP_F32 ? simx_ip_scores(stream, nq, m, H, (const float*)q, (const float*)corpus + c0 * H, (float*)workspace, ld)
                            : ip_scores_h16(what, mode == IP_PLANES, stream, nq, m, H, q16, iph_rows(c16, c0, H), (float*)workspace, ld);
    if (rc) return rc;
    rc = simx_topk_update(stream, nq, m, (const float*)workspace, ld, nullptr, 0, id_base + c0, k, out_scores, out_ids);
    if (rc) return rc;
  }
  return SIMX_OK;
}

extern "C" int simx_flat_ip_search(simx_stream_t stream, int nq, long nc, int H, const float* q, const float* corpus,
                                   int64_t id_base, int k, int chunk, void* workspace, size_t workspace_bytes,
                                   float* out_scores, int64_t* out_ids) {
  return flat_ip_search("flat_ip_search", IP_F32, stream, nq, nc, H, q, nullptr, corpus, nullptr, id_base, k, chunk, workspace, workspace_bytes,
                        out_scores, out_ids);
}

extern "C" int simx_flat_ip_search_f16(simx_stream_t stream, int nq, long nc, int H, const void* q16, const void* corpus16,
                                       int64_t id_base, int k, int chunk, void* workspace, size_t workspace_bytes,
                                       float* out_scores, int64_t* out_ids) {
  return flat_ip_search("flat_ip_search_f16", IP_F16, stream, nq, nc, H, q16, nullptr, corpus16, nullptr, id_base, k, chunk, workspace,
                        workspace_bytes, out_scores, out_ids);
}

extern "C" int simx_flat_ip_search_planes(simx_stream_t stream, int nq, long nc, int H, const void* q_hi, const void* q_lo, const void* corpus_hi,
                                          const void* corpus_lo, int64_t id_base, int k, int chunk, void* workspace, size_t workspace_bytes,
                                          float* out_scores, int64_t* out_ids) {
  return flat_ip_search("flat_ip_search_planes", IP_PLANES, stream, nq, nc, H, q_hi, q_lo, corpus_hi, corpus_lo, id_base, k, chunk, workspace,
                        workspace_bytes, out_scores, out_ids);
}

// ---- one-pass matrix-core search: seed pass unfused, then filter + fold per chunk -------------------------------------------
// workspace: [seed scores nq x ld][cand_scores nq x cap][cand_ids nq x cap][cand_count nq][overflow word], each part 16-byte aligned
struct FusedWs { size_t ld, cand_s, cand_i, count, ovf, total; };
static FusedWs fused_ws(int nq, int seed_rows, int cand_cap) {
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  FusedWs w;
  w.ld = ((size_t)seed_rows + 3) & ~(size_t)3;
  w.cand_s = up((size_t)nq * w.ld * sizeof(float));
  w.cand_i = w.cand_s + up((size_t)nq * cand_cap * sizeof(float));
  w.count = w.cand_i + up((size_t)nq * cand_cap * sizeof(int64_t));
  w.ovf = w.count + up((size_t)nq * sizeof(int));
  w.total = w.ovf + 16;
  return w;
}

extern "C" size_t simx_flat_ip_fused_workspace_bytes(int nq, int seed_rows, int cand_cap) {
  if (nq <= 0 || seed_rows <= 0 || cand_cap <= 0) return 0;
  return fused_ws(nq, seed_rows, cand_cap).total;
}

__global__ void fused_overflow_out_kernel(const int* __restrict__ word, int* __restrict__ out) { *out = *word; }

// the one schedule of both matrix-core modes: seed pass, growing chunks, fold, overflow word
static int flat_ip_search_fused(const char* what, bool planes, simx_stream_t stream, int nq, long nc, int H, IphOperand q, IphOperand corpus,
                                int64_t id_base, int k, int chunk, int seed_rows, int cand_cap, void* workspace, size_t workspace_bytes,
                                float* out_scores, int64_t* out_ids, int* overflow) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(nq > 0 && nc >= 0 && chunk > 0 && seed_rows > 0 && cand_cap > 0, SIMX_ERR_BAD_SHAPE,
               "%s: bad shape nq=%d nc=%ld chunk=%d seed_rows=%d cand_cap=%d", what, nq, nc, chunk, seed_rows, cand_cap);
  SIMX_REQUIRE(H > 0 && H % 8 == 0 && k > 0 && k <= TK_KMAX, SIMX_ERR_BAD_SHAPE, "%s: need H=%d %% 8 == 0 and 0 < k=%d <= %d", what, H, k, TK_KMAX);
  SIMX_REQUIRE(iph_ok(q, planes) && (nc == 0 || iph_ok(corpus, planes)) && workspace && simx_al16(workspace), SIMX_ERR_BAD_SHAPE,
               "%s: queries / corpus / workspace must be non-NULL and 16-byte aligned", what);
  SIMX_REQUIRE(out_scores && out_ids && overflow, SIMX_ERR_BAD_SHAPE, "%s: NULL output", what);
  SIMX_REQUIRE(id_base >= 0 && id_base + nc < 0xFFFFFFFFll, SIMX_ERR_BAD_SHAPE, "%s: ids must fit 32 bits", what);
  SIMX_REQUIRE(workspace_bytes >= simx_flat_ip_fused_workspace_bytes(nq, seed_rows, cand_cap), SIMX_ERR_WORKSPACE, "%s: workspace too small", what);
  const FusedWs w = fused_ws(nq, seed_rows, cand_cap);
  char* base = (char*)workspace;
  float* seed_s = (float*)base;
  float* cand_s = (float*)(base + w.cand_s);
  int64_t* cand_i = (int64_t*)(base + w.cand_i);
  int* count = (int*)(base + w.count);
  int* ovf = (int*)(base + w.ovf);
  hipLaunchKernelGGL(topk_init_kernel, dim3(cdiv((int)((long)nq * k), 256)), dim3(256), 0, s, (long)nq * k, out_scores, (long long*)out_ids);
  SIMX_CHECK_LAUNCH("topk_init");
  if (hipMemsetAsync(count, 0, w.total - w.count, s) != hipSuccess) {          // the counts and the overflow word
    simx_set_error("%s: hipMemsetAsync failed", what);
    return SIMX_ERR_HIP;
  }
  // with an empty running set every score survives: the first seed_rows rows take the unfused pass
  long seen = nc < seed_rows ? nc : seed_rows;
  if (seen > 0) {
    int rc = ip_scores_h16(what, planes, stream, nq, (int)seen, H, q, corpus, seed_s, (long)w.ld);
    if (rc) return rc;
    rc = simx_topk_update(stream, nq, (int)seen, seed_s, (long)w.ld, nullptr, 0, id_base, k, out_scores, out_ids);
    if (rc) return rc;
  }
  // then chunks that grow with what has been seen: about k * m / seen <= k survivors per query on rows in random order
  while (seen < nc) {
    long m = nc - seen;
    if (m > seen) m = seen;
    if (m > chunk) m = chunk;
    int rc = ip_filter_h16(what, planes, stream, nq, (int)m, H, q, iph_rows(corpus, seen, H), id_base + seen, k, out_scores, out_ids, cand_s, cand_i,
                           cand_cap, count);
    if (rc) return rc;
    rc = simx_topk_fold_lists(stream, nq, cand_s, cand_i, cand_cap, count, k, out_scores, out_ids, ovf);
    if (rc) return rc;
    seen += m;
  }
  hipLaunchKernelGGL(fused_overflow_out_kernel, dim3(1), dim3(1), 0, s, ovf, overflow);
  SIMX_CHECK_LAUNCH("fused_overflow_out");
  return SIMX_OK;
}

extern "C" int simx_flat_ip_search_f16_fused(simx_stream_t stream, int nq, long nc, int H, const void* q16, const void* corpus16,
                                             int64_t id_base, int k, int chunk, int seed_rows, int cand_cap, void* workspace,
                                             size_t workspace_bytes, float* out_scores, int64_t* out_ids, int* overflow) {
  return flat_ip_search_fused("flat_ip_search_f16_fused", false, stream, nq, nc, H, IphOperand{(const f16_t*)q16, nullptr},
                              IphOperand{(const f16_t*)corpus16, nullptr}, id_base, k, chunk, seed_rows, cand_cap, workspace, workspace_bytes, out_scores,
                              out_ids, overflow);
}

extern "C" int simx_flat_ip_search_planes_fused(simx_stream_t stream, int nq, long nc, int H, const void* q_hi, const void* q_lo,
                                                const void* corpus_hi, const void* corpus_lo, int64_t id_base, int k, int chunk, int seed_rows,
                                                int cand_cap, void* workspace, size_t workspace_bytes, float* out_scores, int64_t* out_ids,
                                                int* overflow) {
  return flat_ip_search_fused("flat_ip_search_planes_fused", true, stream, nq, nc, H, IphOperand{(const f16_t*)q_hi, (const f16_t*)q_lo},
                              IphOperand{(const f16_t*)corpus_hi, (const f16_t*)corpus_lo}, id_base, k, chunk, seed_rows, cand_cap, workspace,
                              workspace_bytes, out_scores, out_ids, overflow);
}

// ---- mined-negative pool: the device form of the generate job's write_to_file + the rank compute_metrics looks for ------------------
// One wavefront per query over its search-result row (ranks in blocks of 64, lane = rank within the block).  v = the leading
// entries with id >= 0, t = min(top, v).  A rank is a positive when its id is in the query's CSR segment (every lane walks the
// whole segment: no cap on its length; the segment address is wave-uniform).  Negatives are compacted in rank order with a wave
// ballot and a lane prefix count: a count pass (which also finds the first positive rank over all v ranks), then a write pass that
// right-aligns them in [top] columns behind (row 0, +inf) padding.  Positive scores are written slot by slot (the wave looks the
// slot's id up among the first t ranks; unmatched slots get 0), so every output word has exactly one writer: no atomics, no
// pre-zeroing, the output is a pure function of the inputs.
__device__ __forceinline__ bool mn_is_positive(long long id, const long long* __restrict__ pos_ids, int p0, int p1) {
  bool hit = false;
  for (int j = p0; j < p1; ++j) hit |= pos_ids[j] == id;
  return hit;
}

__global__ __launch_bounds__(256) void mine_negatives_kernel(int nq, int k, int top, const float* __restrict__ scores,
                                                             const long long* __restrict__ ids, const int* __restrict__ pos_ptr,
                                                             const long long* __restrict__ pos_ids, int* __restrict__ neg_rows,
                                                             float* __restrict__ neg_scores, int* __restrict__ neg_cnt,
                                                             float* __restrict__ pos_scores, int* __restrict__ first_hit) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;                                       // wave-uniform: the ballots below see whole waves
  const float* S = scores + (long)q * k;
  const long long* I = ids + (long)q * k;
  const int p0 = pos_ptr[q], p1 = pos_ptr[q + 1];
  int v = k;
  for (int b = 0; b * 64 < k; ++b) {
    const int r = b * 64 + lane;
    const unsigned long long m = __ballot(r < k && I[r] < 0);
    if (m) { v = b * 64 + __ffsll((long long)m) - 1; break; }
  }
  const int t = top < v ? top : v;
  // count pass: negatives among the first t ranks, first positive among the first v
  const int last = first_hit ? v : t;
  int c = 0, first = 0;
  for (int b = 0; b * 64 < last; ++b) {
    const int r = b * 64 + lane;
    const bool pos = r < last && mn_is_positive(I[r], pos_ids, p0, p1);
    const unsigned long long m = __ballot(pos);
    if (!first && m) first = b * 64 + __ffsll((long long)m);
    c += __popcll(__ballot(r < t && !pos));
    if (first && (b + 1) * 64 >= t) break;
  }
  if (first_hit && lane == 0) first_hit[q] = first;
  if (pos_scores) {
    for (int j = p0; j < p1; ++j) {
      const long long pid = pos_ids[j];
      bool found = false;
      for (int b = 0; b * 64 < t; ++b) {
        const int r = b * 64 + lane;
        const bool hit = r < t && I[r] == pid;
        if (__ballot(hit)) {
          if (hit) pos_scores[j] = S[r];
          found = true;
          break;
        }
      }
      if (!found && lane == 0) pos_scores[j] = 0.f;
    }
  }
  if (neg_rows) {
    int* rows = neg_rows + (long)q * top;
    float* sc = neg_scores + (long)q * top;
    const int base = top - c;
    for (int i = lane; i < base; i += 64) { rows[i] = 0; sc[i] = INFINITY; }
    int run = 0;
    for (int b = 0; b * 64 < t; ++b) {
      const int r = b * 64 + lane;
      long long id = 0;
      bool neg = false;
      if (r < t) { id = I[r]; neg = !mn_is_positive(id, pos_ids, p0, p1); }
      const unsigned long long m = __ballot(neg);
      if (neg) {
        const int col = base + run + __popcll(m & ((1ull << lane) - 1ull));
        rows[col] = (int)id;
        sc[col] = S[r];
      }
      run += __popcll(m);
    }
    if (lane == 0) neg_cnt[q] = c;
  }
}

// what the host cannot see: flag[0] = an id >= 2^31, flag[1] = pos_ptr does not start at 0 or decreases
__global__ void mine_check_kernel(long n, const long long* __restrict__ ids, int nq, const int* __restrict__ pos_ptr, int* __restrict__ flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && ids[i] >= 0x80000000ll) flag[0] = 1;
  if (i < nq && (pos_ptr[i + 1] < pos_ptr[i] || (i == 0 && pos_ptr[0] != 0))) flag[1] = 1;
}

extern "C" int simx_mine_negatives(simx_stream_t stream, int nq, int k, int top, const float* scores, const int64_t* ids, const int32_t* pos_ptr,
                                   const int64_t* pos_ids, int32_t* neg_rows, float* neg_scores, int32_t* neg_cnt, float* pos_scores,
                                   int32_t* first_hit) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(nq > 0 && k > 0 && k <= TK_KMAX && top > 0 && top <= TK_KMAX, SIMX_ERR_BAD_SHAPE,
               "mine_negatives: need nq=%d > 0, 0 < k=%d <= %d and 0 < top=%d <= %d", nq, k, TK_KMAX, top, TK_KMAX);
  SIMX_REQUIRE(scores && ids && pos_ptr, SIMX_ERR_BAD_SHAPE, "mine_negatives: NULL input (pos_ids may be NULL only when there are no positives)");
  const int n_neg_out = (neg_rows != nullptr) + (neg_scores != nullptr) + (neg_cnt != nullptr);
  SIMX_REQUIRE(n_neg_out == 0 || n_neg_out == 3, SIMX_ERR_BAD_SHAPE, "mine_negatives: neg_rows, neg_scores and neg_cnt come together or not at all");
  SIMX_REQUIRE(n_neg_out || pos_scores || first_hit, SIMX_ERR_BAD_SHAPE, "mine_negatives: no output asked for");
  SIMX_REQUIRE((long)nq * k <= 0x7FFFFFFFl * 256, SIMX_ERR_BAD_SHAPE, "mine_negatives: nq * k too large");
  // the contents the shapes do not show are checked on the device first; one 8-byte read and a stream synchronisation
  int* flag = nullptr;
  int host_flag[2] = {0, 0};
  if (hipMalloc((void**)&flag, sizeof(host_flag)) != hipSuccess) {
    simx_set_error("mine_negatives: hipMalloc of the check word failed");
    return SIMX_ERR_HIP;
  }
  const long n = (long)nq * k;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(host_flag), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mine_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, (const long long*)ids, nq, pos_ptr, flag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_flag, flag, sizeof(host_flag), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(flag);
  if (e != hipSuccess) {
    simx_set_error("mine_negatives: input check failed: %s", hipGetErrorString(e));
    return SIMX_ERR_HIP;
  }
  SIMX_REQUIRE(!host_flag[0], SIMX_ERR_BAD_SHAPE, "mine_negatives: an id is >= 2^31 (rows are stored as int32)");
  SIMX_REQUIRE(!host_flag[1], SIMX_ERR_BAD_SHAPE, "mine_negatives: pos_ptr must start at 0 and never decrease");
  SIMX_PROF(SIMX_K_OTHER, s, (double)nq * (12.0 * k + 8.0 * top));
  hipLaunchKernelGGL(mine_negatives_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, s, nq, k, top, scores, (const long long*)ids, pos_ptr,
                     (const long long*)pos_ids, neg_rows, neg_scores, neg_cnt, pos_scores, first_hit);
  SIMX_CHECK_LAUNCH("mine_negatives");
  return SIMX_OK;
}
