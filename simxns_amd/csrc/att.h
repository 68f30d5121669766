// Shared by the attention units (attention.hip, attention_x3.hip; attention_f32.hip takes the constant and the host part):
//   1. device leaf code of the 16-bit tile image -- 128-B rows of 64 16-bit values, 16-B chunk c of row r stored at chunk
//      c ^ f((r>>1)&7), f = (0,2,4,6,5,7,1,3): conflict-free for both the ds_read_b128 row-fragment pattern and the
//      ds_read_b64_tr_b16 transpose-read pattern;
//   2. the host launch path: one launcher on the per-device LDS limits of common.h, and the compile-time dispatch helper.
// Each kernel's LDS layout is ONE constexpr struct next to the kernel: the kernel takes its offsets from it, the launch its BYTES.
#pragma once
#include <type_traits>
#include "common.h"

#define ATT_LOG2E 1.4426950408889634f

// ---- 1. device ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int att_f(int row) {
  const int i = (row >> 1) & 7;
  return (((i << 1) & 7) + (i >> 2) * 5) & 7;
}
__device__ __forceinline__ int att_off(int row, int c16) { return row * 128 + ((c16 ^ att_f(row)) << 4); }

// stage rows [0, rows_pad) x 64 16-bit values of one head slice by LDS-DMA; rows >= len are clamped copies of row len-1
__device__ __forceinline__ void att_stage(const bf16_t* __restrict__ G, long ld, int len, int rows_pad, char* lds, int wave, int lane,
                                          int nwaves) {
  for (int i = wave; i < (rows_pad >> 3); i += nwaves) {
    const int r = i * 8 + (lane >> 3);
    const int c = (lane & 7) ^ att_f(r);
    const int gr = r < len ? r : len - 1;
    glds16(G + (long)gr * ld + c * 8, lds + i * 1024);
  }
}

__device__ __forceinline__ bf16x8 att_row_frag(const char* tile, int row, int c16) {
  return *reinterpret_cast<const bf16x8*>(tile + att_off(row, c16));
}

// transpose-fragment lane constants of lane 16 fg + fr: the byte offset, inside a 16-row tile, of the lane's ds_read_b64_tr_b16 for
// each of the four 16-column tiles.  The swizzle term does not depend on the 16-row tile index, so a fragment address is
// tile + pair * 4096 + vtr[dt] (+ 2048 for the second tile of the pair).
// (a macro: as a function -- array by reference, or one value per call -- hipcc allocates the registers of the forward kernels
// differently; as text in the kernel the code is the one every kernel was tuned with)
#define ATT_VTR(FR, FG, VTR)                                                                                              \
  do {                                                                                                                    \
    const int rr__ = 4 * (FG) + ((FR) >> 2), tsw__ = att_f(rr__), tx__ = ((FR) & 3) >> 1;                                 \
    _Pragma("unroll") for (int dt__ = 0; dt__ < 4; ++dt__)                                                                \
      (VTR)[dt__] = (uint32_t)(rr__ * 128 + (((dt__ * 2 + tx__) ^ tsw__) << 4) + ((FR) & 1) * 8);                         \
  } while (0)

// LDS reads issued by inline asm (the caller waits ONCE, naming every register in flight).  OFF: a literal byte offset; the O forms
// take any constant expression (they print it in the assembler's own notation)
#define ATT_RD128(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=&v"(DST) : "v"(ADDR) : "memory")
#define ATT_RDTR(DST, ADDR, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:" #OFF : "=&v"(DST) : "v"(ADDR) : "memory")
#define ATT_RD128O(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(DST) : "v"(ADDR), "n"(OFF) : "memory")
#define ATT_RDTRO(DST, ADDR, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=&v"(DST) : "v"(ADDR), "n"(OFF) : "memory")
#define ATT_CAT(LO, HI) ((bf16x8){LO[0], LO[1], LO[2], LO[3], HI[0], HI[1], HI[2], HI[3]})

// ---- 2. host -----------------------------------------------------------------------------------------------------------------
#define ATT_CU_LDS 163840                 // the LDS of a CU: the limit of a kernel whose entry point does not bound its request

// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a compile-time one
template <typename Fn>
auto by_flag(bool flag, Fn&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// Launch Kernel (256 threads) with `bytes` of dynamic LDS, LIMIT the most it is ever launched with.  A limit above 64 KB is a
// per-device kernel attribute: set once per device and kernel (simx_set_lds_attrs), never per launch.  `who` names the entry point.
template <auto Kernel, int LIMIT, typename... Args>
int att_launch_upto(const char* who, hipStream_t s, dim3 grid, size_t bytes, Args... args) {
  static_assert(LIMIT <= ATT_CU_LDS, "more LDS than a CU has");
  bool ok = bytes <= (size_t)LIMIT;
  if constexpr (LIMIT > 65536) {
    static SimxLdsAttrs st;
    static const SimxLdsAttr attr = simx_lds(Kernel, LIMIT);
    ok = ok && simx_set_lds_attrs(st, &attr, 1);
  }
  SIMX_REQUIRE(ok, SIMX_ERR_HIP, "%s: cannot raise dynamic LDS to %zu", who, bytes);
  hipLaunchKernelGGL(Kernel, grid, dim3(256), bytes, s, args...);
  SIMX_CHECK_LAUNCH(who);
  return SIMX_OK;
}
// the same for a kernel whose LDS size is a compile-time constant (its layout struct's BYTES)
template <auto Kernel, int BYTES, typename... Args>
int att_launch(const char* who, hipStream_t s, dim3 grid, Args... args) {
  return att_launch_upto<Kernel, BYTES>(who, s, grid, (size_t)BYTES, args...);
}
