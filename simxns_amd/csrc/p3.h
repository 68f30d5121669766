// The device-side text that the LDS-DMA GEMM units share.  Included by csrc/gemm.hip, gemm_xp.hip, gemm_p5.hip and gemm_tn5.hip.
//   1. common forms -- (xcd_remap and glds16 are in common.h) the V3_* fragment reads / MFMA row / scheduling fence, the P_* global and LDS-DMA
//      accesses, P_LDS: all four units (the V3_* row forms: gemm_nt_h16_v5_kernel, gemm_nt_p3_kernel, gemm_nt_xp_kernel)
//   2. the persistent NT main loop -- p3_half, P_STEP, P_BND_*, the per-tile skeleton: gemm_nt_p3_kernel (gemm.hip) and
//      gemm_nt_xp_kernel (gemm_xp.hip)
//   3. the 256 x 256 TN (wgrad) kernels -- tn2_stage*, TN2_STEP, the ragged-tail zeroing, the slab-store tail: gemm_tn2_kernel
//      (gemm.hip), gemm_tn_xp_kernel and gemm_tn_xq_kernel (gemm_xp.hip); the tail also gemm_tn_h16_kernel (gemm.hip); tn2_acol
//      also gemm_tn5_kernel (gemm_tn5.hip)
//   4. the request / piece forms of the one-wave-per-SIMD kernels: gemm_nt_p5_kernel (gemm_p5.hip), gemm_tn5_kernel (gemm_tn5.hip)
// The loop macros name variables of the kernel that expands them (listed at each section) and expand macros that the kernel
// defines (P_AK / P_BK / P_BND_LAST; TN2_ONE_A / TN2_ONE_B / TN2_BOUNDARY).  A unit #undefs what it defined, nothing of this file.
#pragma once
#include "common.h"

#define V3_READ4(F0, F1, F2, F3, ADDR, O0, O1, O2, O3)                                              \
  asm volatile("ds_read_b128 %0, %4 offset:" #O0 "\n\tds_read_b128 %1, %4 offset:" #O1 "\n\t"       \
               "ds_read_b128 %2, %4 offset:" #O2 "\n\tds_read_b128 %3, %4 offset:" #O3               \
               : "=&v"(F0), "=&v"(F1), "=&v"(F2), "=&v"(F3)                                         \
               : "v"(ADDR)                                                                          \
               : "memory")
#define V3_PIN4(TXT, F0, F1, F2, F3) asm volatile(TXT : "+v"(F0), "+v"(F1), "+v"(F2), "+v"(F3)::"memory")
#define V3_PIN8(TXT, F0, F1, F2, F3, F4, F5, F6, F7) \
  asm volatile(TXT : "+v"(F0), "+v"(F1), "+v"(F2), "+v"(F3), "+v"(F4), "+v"(F5), "+v"(F6), "+v"(F7)::"memory")

// one MFMA row of a 128 x 64 wave tile (acc[8][4], element format F of the expanding kernel), one more fragment read, a scheduling fence
#define V3_MFMA_ROW(I, AF, B0, B1, B2, B3)                                                     \
  acc[I][0] = H16<F>::mfma(B0, AF, acc[I][0]);             \
  acc[I][1] = H16<F>::mfma(B1, AF, acc[I][1]);             \
  acc[I][2] = H16<F>::mfma(B2, AF, acc[I][2]);             \
  acc[I][3] = H16<F>::mfma(B3, AF, acc[I][3])
#define V3_RD1(FR, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=&v"(FR) : "v"(ADDR) : "memory")
#define V3_SB __builtin_amdgcn_sched_barrier(0)

#define V5_STAGE 65536
// ------------------------------------------------------------------------------------------
// Shared by the persistent kernels (gemm_nt_p3_kernel, gemm_nt_xp_kernel, gemm_nt_p5_kernel; P_DMA16 also by the TN kernels):
// 160 KB of dynamic LDS and global accesses in "uniform 64-bit base in SGPRs + 32-bit per-lane offset" form.
// ------------------------------------------------------------------------------------------
#define P_EPI_OFF (2 * V5_STAGE)
#define P_LDS (P_EPI_OFF + 8 * 4096)
// global accesses in "uniform 64-bit base in SGPRs + 32-bit per-lane offset" form: one VGPR per address stream
#define P_GLD4(DST, VOFF, SBASE, OFF) asm volatile("global_load_dwordx4 %0, %1, %2 offset:" #OFF : "=&v"(DST) : "v"(VOFF), "s"(SBASE) : "memory")
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// (the trailing s_nop covers the gfx9 "VMEM store of > 64 bits, then a write of its data VGPRs" hazard, which hipcc's
// hazard recognizer cannot see for a store hidden in inline asm.  One wait state was NOT enough on gfx950: with
// s_nop 0 the first data dword of lanes 12-15 of every 16-lane group was still clobbered by the next VALU write in some
// schedules (tests/test_kernels_gpu.py::test_gemm_nt_persistent caught it) -- the store reads its data 16 lanes x 1 dword per
// cycle; 4 wait states cleared it, 6 are used)
// (the persistent kernel's output stores are non-temporal: the tile is not re-read by this kernel, and with `nt` its lines leave
// the L2 before the operand lines the neighbouring CUs still share -- two-output / N = 3072 shapes 2 % faster, the rest equal;
// "sc0 sc1" (write-through) changes nothing.  SIMX_P3_SAMEC, every tile storing to the same rows so that no store reaches HBM,
// shows what is left: the seven shapes run 6 % faster, QKV 11 % -- a store is acknowledged only when the L2 has room, the 32 CUs
// of an XCD store 4 MB = the whole L2 within a few microseconds, and gfx9's single in-order vmcnt makes the next tile's first
// stage boundary wait for those acknowledgements -- or so it seemed: waiting for the next tile's stage 1 BEFORE the stores
// and passing that first boundary with a bare s_barrier changed nothing (6.73 vs 6.73 ms), so the cost is in the store
// path's back-pressure on the issuing waves themselves.  Skewing the XCDs against each other does not help (per-XCD burst unchanged),
// starting the A panels of an XCD in 4 phase groups (N-tiles of a panel in step) costs its 3/4-tile tail and gains nothing.)
#define SIMX_P3_STORE_BITS " nt"
#define P_GST4(VOFF, SBASE, VAL) asm volatile("global_store_dwordx4 %0, %1, %2" SIMX_P3_STORE_BITS "\n\ts_nop 5" ::"v"(VOFF), "v"(VAL), "s"(SBASE) : "memory")
// LDS-DMA in the same form (M0 = wave-uniform LDS byte address of the 1 KB destination).  The persistent kernel
// uses ONLY this form, so the compiler never tracks M0 in it.
#define P_DMA16(VOFF, SBASE, LDSADDR) \
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(VOFF), "s"(SBASE), "s"(LDSADDR) : "memory")
// ------------------------------------------------------------------------------------------
// Persistent NT kernel, three A stages deep.  tools/vmem_bench shows what bounds the two-stage kernel's main loop: the
// LDS-DMA path delivers ~36 B/clk/CU with two 64 KB stages IN FLIGHT but only ~18 with one, and the two-stage ring has
// exactly one in flight (the other is being consumed) -- throughput = bytes in flight / latency.  Here the A operand
// (activations: HBM / fabric latency, L2 never hits) gets three 32 KB slots, B (weights: L2 hits) two: after a stage
// boundary A(st+2), B(st+2) and A(st+3) are in flight = 96 KB, inside the same 160 KB of LDS.  The epilogue has no LDS
// of its own: it borrows the A slot freed by the tile's last stage -- wave w stages through bytes [4w, 4w+4) KB of that
// slot, which are exactly the bytes wave w's own share of the next A load will overwrite, so each wave re-issues its
// share of that load right after its own epilogue, with no cross-wave synchronisation.
// Every stage boundary waits vmcnt(4): the issue order per wave is ... [B(s+1)(4) A(s+2)(4)] so "all but the 4 youngest"
// = stage s+1 complete.  Needs K >= 256.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void p3_half(const bf16_t* __restrict__ G, int ld, int row0, long k0, uint32_t slot, int wave,
                                        uint32_t off0, uint32_t off1) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = wave * 4 + j;
    const char* sg = reinterpret_cast<const char*>(G + (long)(row0 + i * 8) * ld + k0);
    P_DMA16((j & 1) ? off1 : off0, sg, slot + (uint32_t)(i * 1024));
  }
}

// ---- the main loop of gemm_nt_p3_kernel and gemm_nt_xp_kernel.  The expanding kernel supplies
//   the operands and their geometry: A, lda, B, ldb, wave, lane, wc, fg, nst, lds0, ldsB, offA0/1, offB0/1, oA0/1, oB0/1, bias, bmask;
//   P_AK(S) / P_BK(S): element offset of stream stage S inside a row of A / B (defined before the loop, #undef'd by the kernel);
//   the tile state: m0, n0 (this tile), m0n, n0n (the next), a0, b0 / ac, bc (LDS slots of stage 0 / of the stage being consumed);
//   the registers: acc[8][4], al0-3, ah0-3, bx0-3, by0-3 (fragments), bq0-3 (bias columns);
//   the pending-DMA state, declared by P_PENDING_DMA_STATE: pa_g, pb_g, pa_slot, pb_slot, pa_pend, pb_pend;
//   P_BND_LAST(): the tile's last stage boundary (the epilogue's inputs differ per kernel).
// Epilogue-only per-lane constants are recomputed per tile from a laundered copy of the lane id (P_LANE): left to
// LICM they are hoisted out of the tile loop and stay live (~20 VGPRs) through the main loop, which then spills.
#define P_LANE(L) int L = lane; asm volatile("" : "+v"(L))
// (timing experiments that priced the waits of this loop -- no barrier, no vmcnt wait, no lgkmcnt waits, s_setprio around
// the MFMA bursts, all stores to one tile's rows -- are recorded in DESIGN.md 5 / 5b; the switches are not part of the product)
#define P3_BOUNDARY_WAIT() asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory")
#define P3_LGKM_WAIT "s_waitcnt lgkmcnt(0)"
// the 8 LDS-DMA instructions a mid-tile boundary issues go out ONE PER MFMA ROW (B in the rest of this k-step, A in the
// first half of the next), never as a burst right after the barrier (+5 %)
#define P_PENDING_DMA_STATE                                  \
  const char* pa_g = nullptr; const char* pb_g = nullptr;    \
  uint32_t pa_slot = 0, pb_slot = 0;                         \
  bool pa_pend = false, pb_pend = false
#define P3_HA(J) do { if (pa_pend) { P_DMA16(((J) & 1) ? offA1 : offA0, pa_g + (long)(J) * 8 * lda * 2, pa_slot + (uint32_t)((J) * 1024)); if ((J) == 3) pa_pend = false; } } while (0)
#define P3_HB(J) do { if (pb_pend) { P_DMA16(((J) & 1) ? offB1 : offB0, pb_g + (long)(J) * 8 * ldb * 2, pb_slot + (uint32_t)((J) * 1024)); if ((J) == 3) pb_pend = false; } } while (0)
#define P3_HAX(ROW, S1) do { if ((ROW) < 4) P3_HA(ROW); } while (0)
// one k-step: CURA = this k-step's A-high address, NA / NB = the next k-step's A-low / B addresses; BOUNDARY: what happens
// between the two halves (P_BND_NONE, P_BND_MID, the kernel's P_BND_LAST, gemm_nt_xp_kernel's R_BND*)
#define P_STEP(CURA, NA, NB, BC0, BC1, BC2, BC3, BN0, BN1, BN2, BN3, BOUNDARY, S1)               \
  do {                                                                                         \
    /* fragment reads are front-loaded: the last read before each pin is issued two MFMA rows ahead of it */ \
    const uint32_t aa__ = (CURA), na__ = (NA), nb__ = (NB);                                    \
    V3_SB; V3_MFMA_ROW(0, al0, BC0, BC1, BC2, BC3); V3_SB; V3_RD1(ah0, aa__, 8192); V3_RD1(ah1, aa__, 10240); P3_HAX(0, S1); \
    V3_SB; V3_MFMA_ROW(1, al1, BC0, BC1, BC2, BC3); V3_SB; V3_RD1(ah2, aa__, 12288); V3_RD1(ah3, aa__, 14336); P3_HAX(1, S1); \
    V3_SB; V3_MFMA_ROW(2, al2, BC0, BC1, BC2, BC3); V3_SB; P3_HAX(2, S1);                      \
    V3_SB; V3_MFMA_ROW(3, al3, BC0, BC1, BC2, BC3); V3_SB; P3_HAX(3, S1);                      \
    V3_SB;                                                                                     \
    V3_PIN4(P3_LGKM_WAIT, ah0, ah1, ah2, ah3);                                                 \
    BOUNDARY();                                                                                \
    V3_SB; V3_MFMA_ROW(4, ah0, BC0, BC1, BC2, BC3); V3_SB; V3_RD1(al0, na__, 0); V3_RD1(BN0, nb__, 0); V3_RD1(al1, na__, 2048); P3_HB(1); P3_HAX(4, S1); \
    V3_SB; V3_MFMA_ROW(5, ah1, BC0, BC1, BC2, BC3); V3_SB; V3_RD1(BN1, nb__, 2048); V3_RD1(al2, na__, 4096); V3_RD1(BN2, nb__, 4096); P3_HB(2); P3_HAX(5, S1); \
    V3_SB; V3_MFMA_ROW(6, ah2, BC0, BC1, BC2, BC3); V3_SB; V3_RD1(al3, na__, 6144); V3_RD1(BN3, nb__, 6144); P3_HB(3); P3_HAX(6, S1); \
    V3_SB; V3_MFMA_ROW(7, ah3, BC0, BC1, BC2, BC3);                                            \
    V3_SB;                                                                                     \
    V3_PIN8(P3_LGKM_WAIT, al0, al1, al2, al3, BN0, BN1, BN2, BN3);                             \
  } while (0)
#define P_BND_NONE() do { } while (0)
// stage boundary inside the tile (uses the stage loop's `st`): every fragment of stage st is in registers, stage st+1 has
// landed once vmcnt hits 0 (for everyone after the barrier); slot (st+par)&1 is refilled with stream stage st+2, which is the
// NEXT tile's stage 0 when st == nst-2
#define P_BND_MID()                                                                            \
  do {                                                                                         \
    /* issue order so far: ... [B(st+1) A(st+2)] ; stage st+1 = everything but the 4 youngest (A(st+2)) */ \
    P3_BOUNDARY_WAIT();                                                                        \
    const bool cb__ = st + 2 < nst, ca__ = st + 3 < nst;                                       \
    /* same issue ORDER as a burst would have (B x4, then A x4 -- the vmcnt(4) rule holds), one instruction per MFMA row */ \
    pb_g = reinterpret_cast<const char*>(B + (long)((cb__ ? n0 : n0n) + wave * 32) * ldb + P_BK(cb__ ? st + 2 : st + 2 - nst)); \
    pb_slot = ldsB + (uint32_t)(bc * 32768 + wave * 4096);                                     \
    pa_g = reinterpret_cast<const char*>(A + (long)((ca__ ? m0 : m0n) + wave * 32) * lda + P_AK(ca__ ? st + 3 : st + 3 - nst)); \
    pa_slot = lds0 + (uint32_t)(ac * 32768 + wave * 4096);                                     \
    pb_pend = pa_pend = true;                                                                  \
    P_DMA16(offB0, pb_g, pb_slot);                                                             \
  } while (0)
// head and tail of a kernel's P_BND_LAST (statements, not blocks: `lb__` is the laundered lane id for what the kernel puts
// between them).  The next tile's bias -- and, in between, the epilogue's first input chunk -- are requested BEFORE the next
// tile's stage 1, so the epilogue can wait for them without waiting for that stage.  BPTR: bias + the next tile's columns.
#define P_BND_LAST_HEAD(BPTR)                                                                  \
  asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");                                \
  P_LANE(lb__);                                                                                \
  const uint32_t boff__ = (uint32_t)((lb__ >> 4) * 16);                                        \
  P_GLD4(bq0, boff__, BPTR, 0); P_GLD4(bq1, boff__, BPTR, 64); P_GLD4(bq2, boff__, BPTR, 128); P_GLD4(bq3, boff__, BPTR, 192)
// next tile's stage 1 of B (the kernel issues its first piece); its stage 2 of A goes into the slot this tile's epilogue
// borrows -> issued after it
#define P_BND_LAST_B1()                                                                        \
  pb_g = reinterpret_cast<const char*>(B + (long)(n0n + wave * 32) * ldb + P_BK(1));           \
  pb_slot = ldsB + (uint32_t)(bc * 32768 + wave * 4096)

// the per-tile skeleton around the steps.  The bias enters as the accumulators' initial value; bq* always hold the CURRENT
// tile's 4x4 bias columns at the top of the tile loop (the next tile's are requested at the last stage boundary and carried
// across the epilogue); P_BIAS_FIRST loads the first tile's.
#define P_BIAS_FIRST()                                                                         \
  do {                                                                                         \
    const float* bp0__ = bias ? bias + n0 + wc * 64 : reinterpret_cast<const float*>(A);       \
    const uint32_t boff__ = (uint32_t)(fg * 16);                                                \
    P_GLD4(bq0, boff__, bp0__, 0); P_GLD4(bq1, boff__, bp0__, 64); P_GLD4(bq2, boff__, bp0__, 128); P_GLD4(bq3, boff__, bp0__, 192); \
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(bq0), "+v"(bq1), "+v"(bq2), "+v"(bq3)::"memory"); \
  } while (0)
#define P_ACC_INIT()                                                                           \
  do {                                                                                         \
    f32x4 bi__[4] = {bq0, bq1, bq2, bq3};                                                      \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                              \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) bi__[j][e] = __uint_as_float(__float_as_uint(bi__[j][e]) & bmask); \
    _Pragma("unroll") for (int i = 0; i < 8; ++i)                                              \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = bi__[j];                       \
  } while (0)
// the fragments of the tile's first k-step: AA / AB = fragment addresses of stage 0's A / B slot
#define P_FIRST_FRAGS(AA, AB)                                                                  \
  do {                                                                                         \
    const uint32_t aa__ = (AA), ab__ = (AB);                                                   \
    V3_READ4(al0, al1, al2, al3, aa__, 0, 2048, 4096, 6144);                                   \
    V3_READ4(bx0, bx1, bx2, bx3, ab__, 0, 2048, 4096, 6144);                                   \
    V3_PIN8("s_waitcnt lgkmcnt(0)", al0, al1, al2, al3, bx0, bx1, bx2, bx3);                   \
  } while (0)
// the two k-steps of the stage in slots (ac, bc); BND = the boundary inside the second
#define P_STAGE_ADDR()                                                                         \
  const int an = ac == 2 ? 0 : ac + 1, bn = bc ^ 1;                                            \
  const uint32_t sa = lds0 + (uint32_t)(ac * 32768), sb = ldsB + (uint32_t)(bc * 32768);       \
  const uint32_t na = lds0 + (uint32_t)(an * 32768), nb = ldsB + (uint32_t)(bn * 32768)
#define P_STAGE_STEPS(BND)                                                                     \
  P_STEP(sa + oA0, sa + oA1, sb + oB1, bx0, bx1, bx2, bx3, by0, by1, by2, by3, P_BND_NONE, 1); \
  P_STEP(sa + oA1, na + oA0, nb + oB0, by0, by1, by2, by3, bx0, bx1, bx2, bx3, BND, 0)
// all stages of a tile, the last one peeled; EREG (this wave's slice of the last stage's A slot, which the epilogue borrows)
// is set before it because P_BND_LAST may name it
#define P_TILE_STAGES(EREG)                                                                    \
  do {                                                                                         \
    for (int st = 0; st < nst - 1; ++st) {                                                     \
      P_STAGE_ADDR();                                                                          \
      P_STAGE_STEPS(P_BND_MID);                                                                \
      ac = an; bc = bn;                                                                        \
    }                                                                                          \
    EREG = lds0 + (uint32_t)(ac * 32768 + wave * 4096);                                        \
    {                                                                                          \
      P_STAGE_ADDR();                                                                          \
      P_STAGE_STEPS(P_BND_LAST);                                                               \
    }                                                                                          \
  } while (0)

// ---- the 256x256 TN (wgrad) kernels: stage helpers, main loop, tail (the kernels' own comments: gemm_tn2_kernel, csrc/gemm.hip)
#define TN2_STAGE 65536
#define TN2_LDS (2 * TN2_STAGE)

// (LDS-DMA in the compiler-invisible asm form: with the builtin hipcc assumes every later LDS read may alias the pending
// DMA and waits vmcnt(0) before it; the transpose reads below are BUILTINS so that hipcc allocates both halves of a
// fragment into one 128-bit register tuple and places counted lgkmcnt waits itself -- the inline-asm reads cost 136
// v_mov per stage to assemble the tuples, more VALU time than the MFMAs of a k-step.)
// hm > 0: A is head-major, [M/64][hm][64] (dq/dk/dv, QkvLay in attention.hip): column c of token k sits at
// ((c >> 6) * hm + k) * 64 + (c & 63) -- the row pitch becomes 64 and the column part of the lane offset picks the plane.
__device__ __forceinline__ uint32_t tn2_acol(int c, int hm) { return hm > 0 ? (uint32_t)(c >> 6) * (uint32_t)hm * 64u + (uint32_t)(c & 63) : (uint32_t)c; }
__device__ __forceinline__ void tn2_stage(const bf16_t* __restrict__ A, int lda, int m0, int M,
                                          const bf16_t* __restrict__ B, int ldb, int n0, int N, int k0, int k_end,
                                          char* stage, int wave, int lane, int hm) {
  const uint32_t sbase = (uint32_t)(uintptr_t)stage;
  if (hm > 0) lda = 64;
  const char* ga = reinterpret_cast<const char*>(A + (long)k0 * lda);
  const char* gb = reinterpret_cast<const char*>(B + (long)k0 * ldb);
#pragma unroll
  for (int j = 0; j < 4; ++j) {                 // 32 wave-instructions of 2 k-rows per operand
    const int i = wave * 4 + j;
    const int kr = i * 2 + (lane >> 5);
    const int p16 = lane & 31;
    const int q = (p16 >> 1) ^ (kr & 7);
    int rk = kr;                                 // row relative to k0, clamped into the k-range (ragged tail rows are zeroed later)
    rk = k0 + rk < k_end ? rk : k_end - 1 - k0;
    int ca = m0 + q * 16 + (p16 & 1) * 8, cb = n0 + q * 16 + (p16 & 1) * 8;
    ca = ca + 8 <= M ? ca : M - 8;
    cb = cb + 8 <= N ? cb : N - 8;
    P_DMA16(((uint32_t)(rk * lda) + tn2_acol(ca, hm)) * 2, ga, sbase + (uint32_t)(i * 1024));
    P_DMA16((uint32_t)(rk * ldb + cb) * 2, gb, sbase + (uint32_t)(32768 + i * 1024));
  }
}

// a FULL stage (all 64 k-rows inside the k-range) goes out piece by piece, one LDS-DMA instruction per MFMA row, with the
// per-lane byte offsets precomputed once per kernel (tn2_lane_offsets): the row part of the address rides in the SGPR base, so
// a stage costs no VALU work at all.  tn2_stage above recomputes offsets and clamps per stage (~60 VALU per wave) and is kept
// for the ragged last stage.
__device__ __forceinline__ void tn2_lane_offsets(int lda, int m0, int M, int ldb, int n0, int N, int lane, uint32_t (&oa)[4],
                                                 uint32_t (&ob)[4], int hm) {
  if (hm > 0) lda = 64;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int krl = 2 * j + (lane >> 5);                      // k-row within the wave's 8 rows; (kr & 7) == krl
    const int p16 = lane & 31;
    const int q = (p16 >> 1) ^ (krl & 7);
    int ca = m0 + q * 16 + (p16 & 1) * 8, cb = n0 + q * 16 + (p16 & 1) * 8;
    ca = ca + 8 <= M ? ca : M - 8;
    cb = cb + 8 <= N ? cb : N - 8;
    oa[j] = ((uint32_t)((lane >> 5) * lda) + tn2_acol(ca, hm)) * 2;
    ob[j] = (uint32_t)((lane >> 5) * ldb + cb) * 2;
  }
}
// the wave's j-th instruction of one operand of a full stage (sbase: the operand's 32 KB half of the stage buffer)
__device__ __forceinline__ void tn2_stage_one(const bf16_t* __restrict__ G, int ld, int k0, uint32_t sbase, int wave, int j, uint32_t off) {
  const char* g = reinterpret_cast<const char*>(G + (long)(k0 + wave * 8 + 2 * j) * ld);
  P_DMA16(off, g, sbase + (uint32_t)((wave * 4 + j) * 1024));
}

// one fragment = two transpose reads (k rows base+4g.. and base+16+4g..)
typedef __attribute__((address_space(3))) bf16x4* tn_lds4_t;
#define TN2_RD(F_LO, F_HI, ADDR_LO, ADDR_HI)                                                        \
  do {                                                                                              \
    F_LO = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_lds4_t)(uintptr_t)(ADDR_LO));                \
    F_HI = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_lds4_t)(uintptr_t)(ADDR_HI));                \
  } while (0)

// rows >= VALID of a ragged 64-row stage (both operands) hold clamped copies: zero them, then wait and barrier.  Names tid.
// (a macro: as a function it changes the code around its call sites)
#define TN2_ZERO_TAIL(STAGE, VALID)                                                                             \
  do {                                                                                                          \
    const int valid__ = (VALID);                                                                                \
    char* sp__ = (STAGE);                                                                                       \
    for (int idx = tid; idx < 64 * 64; idx += 512) {                                                            \
      const int kr = idx >> 6, c16 = idx & 63;                                                                  \
      if (kr >= valid__) *reinterpret_cast<uint4*>(sp__ + kr * 512 + (c16 & 31) * 16 + (c16 >> 5) * 32768) = make_uint4(0, 0, 0, 0); \
    }                                                                                                           \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                                             \
  } while (0)

// ---- the main loop of gemm_tn2_kernel and gemm_tn_xp_kernel (gemm_tn_xq_kernel takes the address / fragment / MFMA forms).
// The expanding kernel supplies wr, wc, row_lo, row_hi, x_lo, x_hi (transpose-read addressing), acc[8][4], the fragment halves
// al_lo/al_hi/ah_lo/ah_hi[4], `bool pend`, for the fused bias gradient `do_bias` and bsum[8], and three macros:
//   TN2_ONE_A(ST, J) / TN2_ONE_B(ST, J): piece J of the A / B operand of stream stage ST + 2 into the buffer stage ST leaves;
//   TN2_BOUNDARY(ST, SPREAD): what follows the barrier that ends stage ST -- start stage ST + 2 and zero a ragged stage ST + 1.
//     A full stage ST + 2 is started with TN2_ONE_A(ST, 0) alone and SPREAD = pend = true: the step then issues B0 A1 B1 under
//     its remaining MFMA rows and the next step (pend) A2 B2 A3 B3.
// address of fragment (operand base, 16-col tile ct) for k-step base address `kbase` (stage + ks*32*512)
#define TN2_ADDR_LO(KBASE, OP, CT) ((KBASE) + (OP) + row_lo + (uint32_t)((((CT)) ^ x_lo) << 5))
#define TN2_ADDR_HI(KBASE, OP, CT) ((KBASE) + (OP) + row_hi + (uint32_t)((((CT)) ^ x_hi) << 5))
#define TN2_FRAG(LO, HI) ((bf16x8){LO[0], LO[1], LO[2], LO[3], HI[0], HI[1], HI[2], HI[3]})
#define TN2_MFMA4(I, ALO, AHI, BLO, BHI)                                                                        \
    const bf16x8 af__ = TN2_FRAG(ALO, AHI);                                                                     \
    acc[I][0] = H16<F>::mfma(TN2_FRAG(BLO[0], BHI[0]), af__, acc[I][0]);    \
    acc[I][1] = H16<F>::mfma(TN2_FRAG(BLO[1], BHI[1]), af__, acc[I][1]);    \
    acc[I][2] = H16<F>::mfma(TN2_FRAG(BLO[2], BHI[2]), af__, acc[I][2]);    \
    acc[I][3] = H16<F>::mfma(TN2_FRAG(BLO[3], BHI[3]), af__, acc[I][3])
#define TN2_MFMA_ROW(I, ALO, AHI, BLO, BHI)                                                                     \
  do {                                                                                                          \
    TN2_MFMA4(I, ALO, AHI, BLO, BHI);                                                                           \
    if (do_bias) {                                                                                              \
      _Pragma("unroll") for (int e__ = 0; e__ < 4; ++e__)                                                       \
          bsum[I] += H16<F>::one(ALO[e__]) + H16<F>::one(AHI[e__]);                                           \
    }                                                                                                           \
  } while (0)
#define TN2_SB __builtin_amdgcn_sched_barrier(0)
// (What bounds this loop was priced with timing-only variants, M = 262144 tokens, average of the four wgrad shapes: as shipped
// 992 TFLOP/s; every stage re-reading stage 0 (all L2 hits) 1156; no operand loads at all 1445, 1614 on all-zero data.  So the
// LDS-DMA stream itself costs the loop 20 % and the fabric / HBM misses another 14 %; an L2 prefetch of stage s+3 made it 5 %
// SLOWER.  The 8 DMA instructions of a stage go out ONE PER MFMA ROW after the boundary: burst 1003, one (A,B) pair per row
// 1056, one instruction per row 1080 TFLOP/s.)
// (fragment waits are hipcc's, counted lgkmcnt: the reads are builtins)
// one k-step (32 tokens): CUR = k-step base address, NXT = next k-step base address; SYNC: the stage boundary sits inside
#define TN2_STEP(CUR, NXT, BCL, BCH, BNL, BNH, SYNC, ST)                                                        \
  do {                                                                                                          \
    const uint32_t cur__ = (CUR), nxt__ = (NXT);                                                                \
    bool spread__ = false;                                                                                      \
    const bool tail__ = !(SYNC) && pend;       /* second half of the previous boundary's stage */               \
    TN2_SB; TN2_MFMA_ROW(0, al_lo[0], al_hi[0], BCL, BCH); TN2_SB;                                              \
    TN2_RD(ah_lo[0], ah_hi[0], TN2_ADDR_LO(cur__, 0u, wr * 8 + 4), TN2_ADDR_HI(cur__, 0u, wr * 8 + 4));         \
    TN2_RD(ah_lo[1], ah_hi[1], TN2_ADDR_LO(cur__, 0u, wr * 8 + 5), TN2_ADDR_HI(cur__, 0u, wr * 8 + 5));         \
    if (tail__) TN2_ONE_A((ST) - 1, 2);                                                                         \
    TN2_SB; TN2_MFMA_ROW(1, al_lo[1], al_hi[1], BCL, BCH); TN2_SB;                                              \
    TN2_RD(ah_lo[2], ah_hi[2], TN2_ADDR_LO(cur__, 0u, wr * 8 + 6), TN2_ADDR_HI(cur__, 0u, wr * 8 + 6));         \
    TN2_RD(ah_lo[3], ah_hi[3], TN2_ADDR_LO(cur__, 0u, wr * 8 + 7), TN2_ADDR_HI(cur__, 0u, wr * 8 + 7));         \
    if (tail__) TN2_ONE_B((ST) - 1, 2);                                                                         \
    TN2_SB; TN2_MFMA_ROW(2, al_lo[2], al_hi[2], BCL, BCH);                                                      \
    if (tail__) TN2_ONE_A((ST) - 1, 3);                                                                         \
    TN2_SB; TN2_MFMA_ROW(3, al_lo[3], al_hi[3], BCL, BCH);                                                      \
    if (tail__) { TN2_ONE_B((ST) - 1, 3); pend = false; }                                                       \
    TN2_SB;                                                                                                     \
    if (SYNC) {                                                                                                 \
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");                                             \
      TN2_BOUNDARY(ST, spread__);                                                                               \
    }                                                                                                           \
    TN2_SB; TN2_MFMA_ROW(4, ah_lo[0], ah_hi[0], BCL, BCH); TN2_SB;                                              \
    TN2_RD(al_lo[0], al_hi[0], TN2_ADDR_LO(nxt__, 0u, wr * 8 + 0), TN2_ADDR_HI(nxt__, 0u, wr * 8 + 0));         \
    TN2_RD(BNL[0], BNH[0], TN2_ADDR_LO(nxt__, 32768u, wc * 4 + 0), TN2_ADDR_HI(nxt__, 32768u, wc * 4 + 0));     \
    TN2_RD(al_lo[1], al_hi[1], TN2_ADDR_LO(nxt__, 0u, wr * 8 + 1), TN2_ADDR_HI(nxt__, 0u, wr * 8 + 1));         \
    if (SYNC && spread__) TN2_ONE_B(ST, 0);                                                                     \
    TN2_SB; TN2_MFMA_ROW(5, ah_lo[1], ah_hi[1], BCL, BCH); TN2_SB;                                              \
    TN2_RD(BNL[1], BNH[1], TN2_ADDR_LO(nxt__, 32768u, wc * 4 + 1), TN2_ADDR_HI(nxt__, 32768u, wc * 4 + 1));     \
    TN2_RD(al_lo[2], al_hi[2], TN2_ADDR_LO(nxt__, 0u, wr * 8 + 2), TN2_ADDR_HI(nxt__, 0u, wr * 8 + 2));         \
    TN2_RD(BNL[2], BNH[2], TN2_ADDR_LO(nxt__, 32768u, wc * 4 + 2), TN2_ADDR_HI(nxt__, 32768u, wc * 4 + 2));     \
    if (SYNC && spread__) TN2_ONE_A(ST, 1);                                                                     \
    TN2_SB; TN2_MFMA_ROW(6, ah_lo[2], ah_hi[2], BCL, BCH); TN2_SB;                                              \
    TN2_RD(al_lo[3], al_hi[3], TN2_ADDR_LO(nxt__, 0u, wr * 8 + 3), TN2_ADDR_HI(nxt__, 0u, wr * 8 + 3));         \
    TN2_RD(BNL[3], BNH[3], TN2_ADDR_LO(nxt__, 32768u, wc * 4 + 3), TN2_ADDR_HI(nxt__, 32768u, wc * 4 + 3));     \
    if (SYNC && spread__) TN2_ONE_B(ST, 1);                                                                     \
    TN2_SB; TN2_MFMA_ROW(7, ah_lo[3], ah_hi[3], BCL, BCH);                                                      \
    TN2_SB;                                                                                                     \
  } while (0)
// the fragments of the first k-step of the stage at LDS address S0
#define TN2_FIRST_FRAGS(S0)                                                                                     \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
    TN2_RD(al_lo[i], al_hi[i], TN2_ADDR_LO(S0, 0u, wr * 8 + i), TN2_ADDR_HI(S0, 0u, wr * 8 + i));               \
    TN2_RD(bx_lo[i], bx_hi[i], TN2_ADDR_LO(S0, 32768u, wc * 4 + i), TN2_ADDR_HI(S0, 32768u, wc * 4 + i));       \
  }

// ---- the tail of the TN kernels (macros: as functions they move registers in the 8 x 4 kernels).  The wave's ROWS x 4
// accumulator tiles (16 x 16 each; lane: row fs, columns 4 fg ..) go to the slab / C at O: wave tile of ROWS * 16 rows from MW,
// 64 columns from NW, each value through SCALE(x), on top of what is there if `accumulate`.  Names M, N, ldo, fs, fg, acc.
#define TN_KEEP(X) (X)
#define TN_STORE_TILES(ROWS, O, MW, NW, SCALE)                                                                  \
  _Pragma("unroll") for (int i = 0; i < (ROWS); ++i) {                                                          \
    const int m = (MW) + i * 16 + fs;                                                                           \
    if (m >= M) continue;                                                                                       \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                             \
      const int n = (NW) + j * 16 + fg * 4;                                                                     \
      if (n >= N) continue;                                                                                     \
      float4* dst = reinterpret_cast<float4*>((O) + (long)m * ldo + n);                                         \
      float4 v = make_float4(SCALE(acc[i][j][0]), SCALE(acc[i][j][1]), SCALE(acc[i][j][2]), SCALE(acc[i][j][3])); \
      if (accumulate) { float4 c = *dst; v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w; }                      \
      *dst = v;                                                                                                 \
    }                                                                                                           \
  }
// ... and the fused bias gradient of the 8 x 4 kernels: bsum[i] summed over the four fg groups leaves from the fg == 0 lanes, as
// an atomic on dbias (through SCALE) or, in deterministic mode (dbias_parts), as this wave's row of the ordered partial buffer.
// Names dbias, dbias_parts, bsum, split, bias_mod, bias_slot, m0, wr, M, fs, fg.
#define TN_FLUSH_DBIAS(SCALE)                                                                                   \
  if (dbias != nullptr) {                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                             \
      float t = bsum[i];                                                                                        \
      t += __shfl_xor(t, 16, 64);                                                                               \
      t += __shfl_xor(t, 32, 64);                                                                               \
      const int m = m0 + wr * 128 + i * 16 + fs;                                                                \
      if (fg == 0 && m < M) {                                                                                   \
        if (dbias_parts) dbias[(long)(split * bias_mod + bias_slot) * M + m] = t;                               \
        else atomicAdd(dbias + m, SCALE(t));                                                                    \
      }                                                                                                         \
    }                                                                                                           \
  }

// ---- the request stream of the one-wave-per-SIMD kernels (gemm_nt_p5_kernel, gemm_tn5_kernel; the stream itself is described
// there).  A request = 8 pieces from one base pointer (pA / pB, per-piece lane offsets offA[J] / offB[J]) into this wave's 8 KB
// slice rA / rB of a slot; M0 carries the running LDS address through the pieces (nothing else in those kernels uses M0).  What
// ends a request (the kernel's *_DONE_A / *_DONE_B: advance pointer and slot) differs per kernel.
#define W1_REQ_B() asm volatile("s_mov_b32 m0, %0" ::"s"(rB) : "memory")
#define W1_REQ_A() asm volatile("s_mov_b32 m0, %0" ::"s"(rA) : "memory")
#define W1_PIECE_B(J) asm volatile("global_load_lds_dwordx4 %0, %1\n\ts_add_u32 m0, m0, 0x400" ::"v"(offB[J]), "s"(pB) : "memory", "scc")
#define W1_PIECE_A(J) asm volatile("global_load_lds_dwordx4 %0, %1\n\ts_add_u32 m0, m0, 0x400" ::"v"(offA[J]), "s"(pA) : "memory", "scc")
#define W1_ALL8(M_) do { M_(0); M_(1); M_(2); M_(3); M_(4); M_(5); M_(6); M_(7); } while (0)
