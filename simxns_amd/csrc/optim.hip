// clip_grad_norm_ + transformers.AdamW + zero_grad as two HBM-bound passes over the flat f32 buffers
// (SimANS/co_training/co_training_marco_train.py:57-69, 246-254; update rule SURVEY App. C).
// Pass 1 reads g (4 B/param) for the global L2 norm; pass 2 reads p,g,m,v and writes p,m,v,(g=0):
// 28 (+4) B/param, 16-byte accesses, no host synchronisation (the clip coefficient is computed on
// device from the norm accumulator).
#include "common.h"
#include "prof.h"

// ---- the pieces every kernel below shares, each stated once ------------------------------------------------------------------
// gradient multiplier: 1/W of the data-parallel mean times clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)) from the device scalar
__device__ __forceinline__ float clip_coef(const float* sqnorm, float max_norm, float grad_scale) {
  float coef = grad_scale;
  if (sqnorm && max_norm > 0.f) {
    const float total = sqrtf(*sqnorm) * grad_scale;
    coef *= fminf(1.0f, max_norm / (total + 1e-6f));
  }
  return coef;
}
// the loss scaler (state below; NULL: none) found an overflow: this step leaves parameters and moments alone
__device__ __forceinline__ bool scaler_skips(const float* scaler) { return scaler && scaler[3] != 0.f; }
// g[0, n) = 0 over the grid-stride walk of adamw_kernel (float4 i to thread i mod 256 of block i / 256 mod grid, the n % 4 tail
// elements to block 0): what a step the loss scaler skips still does
__device__ __forceinline__ void zero_grads(float* __restrict__ g, size_t n) {
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) st4(g + 4 * i, zero);
  if (blockIdx.x == 0) for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) g[i] = 0.f;
}
// 256-thread blocks, one float4 per thread and pass, at most `cap` blocks (the kernels stride over the rest)
static unsigned grid_for(size_t n, size_t cap) {
  const size_t blocks = (n / 4 + 255) / 256;
  return (unsigned)(blocks > cap ? cap : blocks < 1 ? 1 : blocks);
}

// Squared L2 norm: ONE body; the block's sum leaves either as a float atomic into `out` or, deterministic variant, as partial
// blockIdx.x for sqnorm_final_kernel (one block) to add in index order.  No float atomics there: every rank of a data-parallel job
// gets the SAME bits from the same all-reduced gradients, so the clip coefficient -- and with it the replicas -- cannot drift apart.
template <bool ATOMIC>
__device__ __forceinline__ void sqnorm_body(const float* __restrict__ g, size_t n, float* __restrict__ out) {
  float s[1] = {0.f}, v[4];
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    ld4(g + 4 * i, v);
    s[0] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0) for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) s[0] += g[i] * g[i];
  block_sum256(s);
  if (threadIdx.x != 0) return;
  if constexpr (ATOMIC) atomicAdd(out, s[0]); else out[blockIdx.x] = s[0];
}
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, size_t n, float* __restrict__ out) {
  sqnorm_body<true>(g, n, out);
}
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partials) {
  sqnorm_body<false>(g, n, partials);
}
__global__ __launch_bounds__(256) void sqnorm_final_kernel(const float* __restrict__ partials, int nparts, float* __restrict__ out) {
  float s[1] = {0.f};
  for (int i = threadIdx.x; i < nparts; i += 256) s[0] += partials[i];
  block_sum256(s);
  if (threadIdx.x == 0) *out += s[0];
}

// Dynamic loss scaler of the fp16 engine (apex.amp's dynamic loss scaling, which the reference's --fp16 mode runs under:
// SimANS/co_training/co_training_marco_train.py:97-104, 218-220; apex defaults: start 2^16, halve on overflow, double after
// 2000 clean steps, cap 2^24).  State, 8 floats on the device:
//   [0] S   [1] 1/S   [2] clean steps since S last changed   [3] 1 = skip the current optimiser step (overflow)
//   [4] optimiser steps applied   [5] steps skipped   [6] growth interval   [7] largest S
// The gradient buffers hold TRUE gradients (every accumulating kernel multiplies by 1/S), so an overflow of the scaled fp16
// activation gradients shows as inf / nan in the squared norm.  No host synchronisation: the AdamW kernel reads [3], [4].
__global__ void scaler_init_kernel(float* __restrict__ st, float init_scale, float growth_interval, float max_scale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st[0] = init_scale; st[1] = 1.0f / init_scale; st[2] = 0.f; st[3] = 0.f; st[4] = 0.f; st[5] = 0.f; st[6] = growth_interval; st[7] = max_scale;
}
__global__ void scaler_update_kernel(float* __restrict__ st, const float* __restrict__ sqnorm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float sq = *sqnorm;
  const bool ok = sq == sq && sq < 3.0e38f && sq >= 0.f;
  float S = st[0];
  if (!ok) {
    S = fmaxf(S * 0.5f, 1.0f);
    st[2] = 0.f; st[3] = 1.f; st[5] += 1.f;
  } else {
    st[3] = 0.f; st[4] += 1.f;
    const float clean = st[2] + 1.f;
    if (st[6] > 0.f && clean >= st[6]) { S = fminf(S * 2.0f, st[7]); st[2] = 0.f; } else st[2] = clean;
  }
  st[0] = S;
  st[1] = 1.0f / S;
}

// m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g g, the ONE statement for AdamW and LAMB.  Left to contraction the compiler fuses
// one product in a float4 body and another (or none) in a scalar head or tail, which round differently; spelled out, in the form
// the float4 bodies have always had, an element gets the same bits wherever it sits in a buffer.
__device__ __forceinline__ void moments(float& m, float& v, float gg, float beta1, float beta2, float omb1, float omb2) {
  m = __fmaf_rn(beta1, m, omb1 * gg);
  v = __fmaf_rn(omb2 * gg, gg, beta2 * v);
}
// transformers.AdamW on one element: moments, bias-corrected step, then the decoupled decay of the UPDATED parameter
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float coef, float step_size, float beta1, float beta2,
                                           float eps, float decay) {
  const float gg = g * coef;
  moments(m, v, gg, beta1, beta2, 1.0f - beta1, 1.0f - beta2);
  p = p - step_size * m / (sqrtf(v) + eps);
  p = __fmaf_rn(-decay, p, p);
}
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n, float step_size, float beta1, float beta2,
                                                    float eps, float decay, const float* __restrict__ sqnorm, float max_norm,
                                                    float grad_scale, int zero_grad, const float* __restrict__ scaler, float lr) {
  const float coef = clip_coef(sqnorm, max_norm, grad_scale);
  if (scaler) {
    // the step count that enters the bias correction is the number of steps APPLIED (skipped ones do not age the moments)
    const double t = (double)scaler[4];
    step_size = (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t)));
    if (scaler_skips(scaler)) {                    // overflow: parameters and moments keep their values, gradients are dropped
      if (zero_grad) zero_grads(g, n);
      return;
    }
  }
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float pv[4], gv[4], mv[4], vv[4];
    ld4(p + 4 * i, pv); ld4(g + 4 * i, gv); ld4(m + 4 * i, mv); ld4(v + 4 * i, vv);
#pragma unroll
    for (int e = 0; e < 4; ++e) adamw_elem(pv[e], gv[e], mv[e], vv[e], coef, step_size, beta1, beta2, eps, decay);
    st4(p + 4 * i, pv); st4(m + 4 * i, mv); st4(v + 4 * i, vv);
    if (zero_grad) st4(g + 4 * i, zero);
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
      adamw_elem(p[i], g[i], m[i], v[i], coef, step_size, beta1, beta2, eps, decay);
      if (zero_grad) g[i] = 0.f;
    }
}

extern "C" int simx_sqnorm_accum(simx_stream_t stream, const float* g, size_t n, float* sqnorm) {
  SIMX_PROF(SIMX_K_ADAMW, stream, 4.0 * n);
  SIMX_REQUIRE(g && sqnorm && n > 0, SIMX_ERR_BAD_SHAPE, "sqnorm_accum: bad arguments");
  SIMX_REQUIRE(simx_al16(g), SIMX_ERR_BAD_SHAPE, "sqnorm_accum: g not 16-B aligned");
  hipLaunchKernelGGL(sqnorm_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, (hipStream_t)stream, g, n, sqnorm);
  SIMX_CHECK_LAUNCH("sqnorm");
  return SIMX_OK;
}

extern "C" int simx_sqnorm_accum_det(simx_stream_t stream, const float* g, size_t n, float* sqnorm, float* ws) {
  SIMX_PROF(SIMX_K_ADAMW, stream, 4.0 * n);
  SIMX_REQUIRE(g && sqnorm && ws && n > 0, SIMX_ERR_BAD_SHAPE, "sqnorm_accum_det: bad arguments");
  SIMX_REQUIRE(simx_al16(g), SIMX_ERR_BAD_SHAPE, "sqnorm_accum_det: g not 16-B aligned");
  const unsigned blocks = grid_for(n, SIMX_SQNORM_WS_FLOATS);
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, ws);
  SIMX_CHECK_LAUNCH("sqnorm_partial");
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, (int)blocks, sqnorm);
  SIMX_CHECK_LAUNCH("sqnorm_final");
  return SIMX_OK;
}

extern "C" int simx_scaler_init(simx_stream_t stream, float* state, float init_scale, float growth_interval, float max_scale) {
  SIMX_REQUIRE(state && init_scale >= 1.f && max_scale >= init_scale, SIMX_ERR_BAD_SHAPE, "scaler_init: bad arguments");
  hipLaunchKernelGGL(scaler_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, init_scale, growth_interval, max_scale);
  SIMX_CHECK_LAUNCH("scaler_init");
  return SIMX_OK;
}
extern "C" int simx_scaler_update(simx_stream_t stream, float* state, const float* sqnorm) {
  SIMX_REQUIRE(state && sqnorm, SIMX_ERR_BAD_SHAPE, "scaler_update: bad arguments");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sqnorm);
  SIMX_CHECK_LAUNCH("scaler_update");
  return SIMX_OK;
}

extern "C" int simx_adamw_step(simx_stream_t stream, float* p, float* g, float* m, float* v, size_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int step, const float* sqnorm, float max_norm,
                               float grad_scale, int zero_grad) {
  return simx_adamw_step_sc(stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, sqnorm, max_norm, grad_scale, zero_grad,
                            nullptr);
}
extern "C" int simx_adamw_step_sc(simx_stream_t stream, float* p, float* g, float* m, float* v, size_t n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int step, const float* sqnorm, float max_norm,
                                  float grad_scale, int zero_grad, const float* scaler) {
  SIMX_PROF(SIMX_K_ADAMW, stream, 32.0 * n);
  SIMX_REQUIRE(p && g && m && v && n > 0 && step >= 1, SIMX_ERR_BAD_SHAPE, "adamw_step: bad arguments");
  SIMX_REQUIRE(simx_al16(p) && simx_al16(g) && simx_al16(m) && simx_al16(v), SIMX_ERR_BAD_SHAPE, "adamw_step: buffers not 16-B aligned");
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr * sqrt(bc2) / bc1);
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, step_size, beta1,
                     beta2, eps, lr * weight_decay, sqnorm, max_norm, grad_scale, zero_grad, scaler, lr);
  SIMX_CHECK_LAUNCH("adamw");
  return SIMX_OK;
}

// ---------------------------------------------------------------------------------------------- LAMB
// PROD/ProD_KD/utils/lamb.py:60-123 (the Lamb of get_optimizer's --optimizer lamb) over a flat f32 buffer.  The update of every
// parameter tensor ("segment") is scaled by its trust ratio min(|p|, 10) / |u|, u = m / (sqrt(v) + eps) + wd * p, so the buffer is
// cut into chunks of at most SIMX_LAMB_CHUNK elements that never cross a segment boundary:
//   pass A   (one workgroup per chunk)  m, v updated and stored; sum p^2 and sum u^2 of the chunk -> partials[2c], [2c + 1]
//   finalize (one wave per segment)     partials added in a fixed order -> stats[seg] = {weight_norm, adam_norm, trust_ratio}
//   pass B   (one workgroup per chunk)  u recomputed from the unchanged p and the stored m, v; p -= lr * ratio * u; g = 0
// 44 B/param (A: 16 read + 8 written, B: 12 + 8).  No float atomics and a fixed element -> thread -> lane order in every sum, so
// the replicas of a data-parallel job get the same bits; no host read; on a step the fp16 loss scaler skips only g is written.
// lamb_u is the ONE statement of u: both passes must round it alike, so the multiply-add is spelled out, not left to contraction.
__device__ __forceinline__ float lamb_u(float p, float m, float v, float eps, float wd) {
  return __fmaf_rn(wd, p, m / (sqrtf(v) + eps));
}
__device__ __forceinline__ bool lamb_chunk_ok(const simx_lamb_chunk_t& c, size_t n, int nseg) {
  return c.seg >= 0 && c.seg < nseg && c.len > 0 && c.len <= SIMX_LAMB_CHUNK && c.off >= 0 && (size_t)c.off + (size_t)c.len <= n;
}
// scalar head up to 16-byte alignment (the buffers are 16-B aligned, so that is the element offset mod 4), float4 body, scalar tail
__device__ __forceinline__ void lamb_split(const simx_lamb_chunk_t& c, int& head, int& body4) {
  head = (int)((4 - (c.off & 3)) & 3);
  if (head > c.len) head = c.len;
  body4 = (c.len - head) / 4;
}

// the head and tail elements of a chunk, one per thread each (head < 4, tail < 4)
template <typename F>
__device__ __forceinline__ void lamb_edges(const simx_lamb_chunk_t& c, int head, int body4, F one) {
  if ((int)threadIdx.x < head) one(threadIdx.x);
  const int t0 = head + body4 * 4;
  if (t0 + (int)threadIdx.x < c.len) one(t0 + threadIdx.x);
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, size_t n, const simx_lamb_chunk_t* __restrict__ chunks,
                                                           const float* __restrict__ seg_wd, int nseg, float* __restrict__ partials,
                                                           float beta1, float beta2, float omb1, float omb2, float eps,
                                                           const float* __restrict__ sqnorm, float max_norm, float grad_scale, const float* __restrict__ scaler) {
  if (scaler_skips(scaler)) return;
  const simx_lamb_chunk_t c = chunks[blockIdx.x];
  if (!lamb_chunk_ok(c, n, nseg)) return;
  const float coef = clip_coef(sqnorm, max_norm, grad_scale), wd = seg_wd[c.seg];
  int head, body4;
  lamb_split(c, head, body4);
  p += c.off; g += c.off; m += c.off; v += c.off;
  float s[2] = {0.f, 0.f};                                   // sum p^2, sum u^2 of the chunk
  auto elem = [&](float pe, float ge, float& me, float& ve) {      // the moments of one element, and its share of the two sums
    moments(me, ve, ge * coef, beta1, beta2, omb1, omb2);
    const float u = lamb_u(pe, me, ve, eps, wd);
    s[0] += pe * pe; s[1] += u * u;
  };
  for (int i = threadIdx.x; i < body4; i += 256) {
    float pv[4], gv[4], mv[4], vv[4];
    ld4(p + head + 4 * i, pv); ld4(g + head + 4 * i, gv); ld4(m + head + 4 * i, mv); ld4(v + head + 4 * i, vv);
#pragma unroll
    for (int e = 0; e < 4; ++e) elem(pv[e], gv[e], mv[e], vv[e]);
    st4(m + head + 4 * i, mv); st4(v + head + 4 * i, vv);
  }
  lamb_edges(c, head, body4, [&](int i) { elem(p[i], g[i], m[i], v[i]); });
  block_sum256(s);
  if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = s[0]; partials[2 * (size_t)blockIdx.x + 1] = s[1]; }
}

__global__ __launch_bounds__(64) void lamb_ratio_kernel(const float* __restrict__ partials, const int* __restrict__ seg_chunks, int nchunk,
                                                        float* __restrict__ stats, const float* __restrict__ scaler) {
  if (scaler_skips(scaler)) return;
  const int first = seg_chunks[2 * blockIdx.x], count = seg_chunks[2 * blockIdx.x + 1];
  if (first < 0 || count < 1 || first > nchunk - count) return;
  float sp = 0.f, su = 0.f;
  for (int i = threadIdx.x; i < count; i += 64) {          // lane l adds chunks l, l + 64, ... in chunk order; then the fixed lane tree
    sp += partials[2 * (size_t)(first + i)];
    su += partials[2 * (size_t)(first + i) + 1];
  }
  sp = wave_sum(sp); su = wave_sum(su);
  if (threadIdx.x == 0) {
    const float wn = fminf(sqrtf(sp), 10.0f), an = sqrtf(su);
    float* st = stats + 3 * (size_t)blockIdx.x;
    st[0] = wn; st[1] = an; st[2] = (wn == 0.f || an == 0.f) ? 1.0f : wn / an;
  }
}

__global__ __launch_bounds__(256) void lamb_update_kernel(float* __restrict__ p, float* __restrict__ g, const float* __restrict__ m,
                                                          const float* __restrict__ v, size_t n, const simx_lamb_chunk_t* __restrict__ chunks,
                                                          const float* __restrict__ seg_wd, int nseg, const float* __restrict__ stats,
                                                          float lr, float eps, int zero_grad, const float* __restrict__ scaler) {
  const simx_lamb_chunk_t c = chunks[blockIdx.x];
  if (!lamb_chunk_ok(c, n, nseg)) return;
  const bool skip = scaler_skips(scaler);                    // overflow: parameters, moments and stats keep their bits
  if (skip && !zero_grad) return;
  int head, body4;
  lamb_split(c, head, body4);
  p += c.off; g += c.off; m += c.off; v += c.off;
  const float wd = seg_wd[c.seg];
  const float ns = skip ? 0.f : -(lr * stats[3 * (size_t)c.seg + 2]);
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  auto elem = [&](float& pe, float me, float ve) { pe = __fmaf_rn(ns, lamb_u(pe, me, ve, eps, wd), pe); };
  for (int i = threadIdx.x; i < body4; i += 256) {
    if (!skip) {
      float pv[4], mv[4], vv[4];
      ld4(p + head + 4 * i, pv); ld4(m + head + 4 * i, mv); ld4(v + head + 4 * i, vv);
#pragma unroll
      for (int e = 0; e < 4; ++e) elem(pv[e], mv[e], vv[e]);
      st4(p + head + 4 * i, pv);
    }
    if (zero_grad) st4(g + head + 4 * i, zero);
  }
  lamb_edges(c, head, body4, [&](int i) {
    if (!skip) elem(p[i], m[i], v[i]);
    if (zero_grad) g[i] = 0.f;
  });
}

extern "C" int simx_lamb_chunk(void) { return SIMX_LAMB_CHUNK; }

extern "C" int simx_lamb_plan_check(const simx_lamb_chunk_t* chunks, int nchunk, const int* seg_chunks, const int64_t* seg_range,
                                    int nseg, size_t n) {
  SIMX_REQUIRE(chunks && seg_chunks && seg_range, SIMX_ERR_BAD_SHAPE, "lamb_plan_check: null table");
  SIMX_REQUIRE(nseg >= 1 && nchunk >= nseg && n > 0, SIMX_ERR_BAD_SHAPE, "lamb_plan_check: nseg %d, nchunk %d, n %zu", nseg, nchunk, n);
  int next = 0;
  long long end_prev = 0;
  for (int s = 0; s < nseg; ++s) {
    const int first = seg_chunks[2 * s], count = seg_chunks[2 * s + 1];
    const long long lo = (long long)seg_range[2 * s], len = (long long)seg_range[2 * s + 1];
    SIMX_REQUIRE(lo >= end_prev && len >= 1 && (size_t)(lo + len) <= n, SIMX_ERR_BAD_SHAPE,
                 "lamb_plan_check: segment %d [%lld, +%lld) overlaps its predecessor or leaves the buffer of %zu", s, lo, len, n);
    SIMX_REQUIRE(first == next && count >= 1 && count <= nchunk - first, SIMX_ERR_BAD_SHAPE,
                 "lamb_plan_check: segment %d owns chunks [%d, +%d), expected them to start at %d", s, first, count, next);
    long long at = lo;
    for (int c = first; c < first + count; ++c) {
      SIMX_REQUIRE(chunks[c].seg == s && chunks[c].off == at && chunks[c].len >= 1 && chunks[c].len <= SIMX_LAMB_CHUNK &&
                   at + chunks[c].len <= lo + len, SIMX_ERR_BAD_SHAPE,
                   "lamb_plan_check: chunk %d (segment %d, offset %lld, %d elements) crosses or leaves segment %d [%lld, +%lld)", c,
                   chunks[c].seg, (long long)chunks[c].off, chunks[c].len, s, lo, len);
      at += chunks[c].len;
    }
    SIMX_REQUIRE(at == lo + len, SIMX_ERR_BAD_SHAPE, "lamb_plan_check: the chunks of segment %d cover %lld of its %lld elements", s, at - lo, len);
    next = first + count;
    end_prev = lo + len;
  }
  SIMX_REQUIRE(next == nchunk, SIMX_ERR_BAD_SHAPE, "lamb_plan_check: %d chunks belong to no segment", nchunk - next);
  return SIMX_OK;
}

extern "C" int simx_lamb_step(simx_stream_t stream, float* p, float* g, float* m, float* v, size_t n, const simx_lamb_chunk_t* chunks,
                              int nchunk, const int* seg_chunks, const float* seg_wd, int nseg, float* stats, float* partials, float lr,
                              double beta1, double beta2, float eps, const float* sqnorm, float max_norm, float grad_scale, int zero_grad,
                              const float* scaler) {
  SIMX_PROF(SIMX_K_ADAMW, stream, 44.0 * n);
  SIMX_REQUIRE(p && g && m && v && chunks && seg_chunks && seg_wd && stats && partials, SIMX_ERR_BAD_SHAPE, "lamb_step: null pointer");
  SIMX_REQUIRE(n > 0 && nseg >= 1 && nchunk >= nseg, SIMX_ERR_BAD_SHAPE, "lamb_step: n %zu, nseg %d, nchunk %d", n, nseg, nchunk);
  // (1 - beta in double, rounded once: the reference hands Python's 1 - beta to the tensor op, and 1.0f - 0.999f is off by 5e-5 of itself)
  SIMX_REQUIRE(simx_al16(p) && simx_al16(g) && simx_al16(m) && simx_al16(v) && simx_al16(chunks), SIMX_ERR_BAD_SHAPE,
               "lamb_step: buffers not 16-B aligned");
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, (const float*)p, (const float*)g, m, v,
                     n, chunks, seg_wd, nseg, partials, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, sqnorm, max_norm,
                     grad_scale, scaler);
  SIMX_CHECK_LAUNCH("lamb_moments");
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, (const float*)partials, seg_chunks, nchunk,
                     stats, scaler);
  SIMX_CHECK_LAUNCH("lamb_ratio");
  hipLaunchKernelGGL(lamb_update_kernel, dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, p, g, (const float*)m, (const float*)v,
                     n, chunks, seg_wd, nseg, (const float*)stats, lr, eps, zero_grad, scaler);
  SIMX_CHECK_LAUNCH("lamb_update");
  return SIMX_OK;
}
