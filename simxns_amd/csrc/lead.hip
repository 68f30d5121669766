// LEAD layer-score distillation (LEAD/util.py:540-831, distill_loss with distill_de / distill_db / distill_de_db_layer_score):
// n slots of (student, teacher) all-pairs scores S = q ctx^T, Z = tq tctx^T, each slot the mutual objective
//   a NLL(S) + b NLL(Z) + w KL(softmax(Z/T) || softmax(S)) + x KL(softmax(S/T) || softmax(Z)),
// differentiated through BOTH arguments of every KL, w of the flagged slots a softmax over their teacher NLLs.
//   lead_row_stats_kernel : one wave per (slot, row): the four log-sum-exps and the four row losses, S and Z read once each pass
//   lead_reduce_kernel    : one workgroup: per-slot means in a fixed order, lambda, weights, total -- no atomics, no host read
//   lead_grad_kernel      : one wave per (slot, row): S <- dS and (teacher_grad) Z <- dZ in place, w read from `weights`
// The score products and the four backward products are the exact-f32 strided GEMM of the other all-pairs losses (loss.hip).
#include "common.h"

struct lead_slots { simx_lead_slot s[SIMX_LEAD_MAX_SLOTS]; };
constexpr int LEAD_STATS = 8;      // per (slot, row): lse(S), lse(S/T), lse(Z), lse(Z/T), nll_s, nll_t, kl_ts, kl_st

__global__ __launch_bounds__(256) void lead_row_stats_kernel(int Q, int C, const float* __restrict__ S, const float* __restrict__ Z,
                                                             const int* __restrict__ pos_idx, float iT, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w, slot = blockIdx.y;
  if (i >= Q) return;
  const long row = (long)slot * Q + i;
  const float* s = S + row * C;
  const float* z = Z + row * C;
  float ms = -INFINITY, mz = -INFINITY;
  for (int c = lane; c < C; c += 64) { ms = fmaxf(ms, s[c]); mz = fmaxf(mz, z[c]); }
  ms = wave_max(ms); mz = wave_max(mz);
  float e1 = 0.f, eT = 0.f, z1 = 0.f, zT = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float ds = s[c] - ms, dz = z[c] - mz;
    e1 += expf(ds); eT += expf(ds * iT);
    z1 += expf(dz); zT += expf(dz * iT);
  }
  e1 = wave_sum(e1); eT = wave_sum(eT); z1 = wave_sum(z1); zT = wave_sum(zT);
  const float lseS = ms + logf(e1), lseST = ms * iT + logf(eT), lseZ = mz + logf(z1), lseZT = mz * iT + logf(zT);
  float kts = 0.f, kst = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float sv = s[c], zv = z[c];
    const float lp = sv - lseS, lv = sv * iT - lseST, lr = zv - lseZ, lu = zv * iT - lseZT;
    const float u = expf(lu), v = expf(lv);
    if (u > 0.f) kts += u * (lu - lp);                  // 0 log 0 = 0 (F.kl_div)
    if (v > 0.f) kst += v * (lv - lr);
  }
  kts = wave_sum(kts); kst = wave_sum(kst);
  if (lane == 0) {
    const int pos = pos_idx[i];
    float4* o = reinterpret_cast<float4*>(stats + row * LEAD_STATS);
    o[0] = make_float4(lseS, lseST, lseZ, lseZT);
    o[1] = make_float4(lseS - s[pos], lseZ - z[pos], kts, kst);
  }
}

// wave w adds the rows of slots w, w + 4, ... (lane-strided partial sums, then the wave tree: one fixed order); thread 0 then
// forms lambda = softmax_i(-nll_t,i / layer_temperature) over the flagged slots, the applied weights and the total
__global__ __launch_bounds__(256) void lead_reduce_kernel(int n, int Q, const float* __restrict__ stats, lead_slots sl, float iLT,
                                                          float lscale, float* __restrict__ slot_losses, float* __restrict__ weights,
                                                          float* __restrict__ total) {
  __shared__ float sums[SIMX_LEAD_MAX_SLOTS][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float invQ = 1.0f / (float)Q;
  for (int slot = w; slot < n; slot += 4) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = lane; i < Q; i += 64) {
      const float4 v = *reinterpret_cast<const float4*>(stats + ((long)slot * Q + i) * LEAD_STATS + 4);
      a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    a0 = wave_sum(a0) * invQ; a1 = wave_sum(a1) * invQ; a2 = wave_sum(a2) * invQ; a3 = wave_sum(a3) * invQ;
    if (lane == 0) {
      sums[slot][0] = a0; sums[slot][1] = a1; sums[slot][2] = a2; sums[slot][3] = a3;
      *reinterpret_cast<float4*>(slot_losses + 4L * slot) = make_float4(a0, a1, a2, a3);
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float mx = -INFINITY, den = 0.f, tot = 0.f;
  for (int i = 0; i < n; ++i)
    if (sl.s[i].reweight) mx = fmaxf(mx, -sums[i][1] * iLT);
  for (int i = 0; i < n; ++i)
    if (sl.s[i].reweight) den += expf(-sums[i][1] * iLT - mx);
  for (int i = 0; i < n; ++i) {
    const float wi = sl.s[i].reweight ? expf(-sums[i][1] * iLT - mx) / den : sl.s[i].w;
    weights[i] = wi;
    tot += sl.s[i].a * sums[i][0] + sl.s[i].b * sums[i][1] + wi * sums[i][2] + sl.s[i].x * sums[i][3];
  }
  *total = tot * lscale;
}

// dS = gscale [ a (p - e_pos) + w (p - u) + (x/T) v (h - sum_c v h) ],  h = log v - log r   (sum_c v h = the row's kl_st)
// dZ = gscale [ b (r - e_pos) + x (r - v) + (w/T) u (g - sum_c u g) ],  g = log u - log p   (sum_c u g = the row's kl_ts)
__global__ __launch_bounds__(256) void lead_grad_kernel(int Q, int C, float* __restrict__ S, float* __restrict__ Z,
                                                        const int* __restrict__ pos_idx, float iT, lead_slots sl,
                                                        const float* __restrict__ weights, const float* __restrict__ stats,
                                                        float gscale, int teacher_grad) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, slot = blockIdx.y;
  if (i >= Q) return;
  const long row = (long)slot * Q + i;
  float* s = S + row * C;
  float* z = Z + row * C;
  const float a = sl.s[slot].a, b = sl.s[slot].b, x = sl.s[slot].x, w = weights[slot];
  const float4 lse = *reinterpret_cast<const float4*>(stats + row * LEAD_STATS);
  const float4 rl = *reinterpret_cast<const float4*>(stats + row * LEAD_STATS + 4);
  const int pos = pos_idx[i];
  for (int c = lane; c < C; c += 64) {
    const float sv = s[c], zv = z[c];
    const float lp = sv - lse.x, lv = sv * iT - lse.y, lr = zv - lse.z, lu = zv * iT - lse.w;
    const float p = expf(lp), v = expf(lv), r = expf(lr), u = expf(lu);
    const float hot = c == pos ? 1.f : 0.f;
    s[c] = gscale * (a * (p - hot) + w * (p - u) + x * iT * v * ((lv - lr) - rl.w));
    if (teacher_grad) z[c] = gscale * (b * (r - hot) + x * (r - v) + w * iT * u * ((lu - lp) - rl.z));
  }
}

static size_t lead_stats_bytes(int n, int Q) { return (((size_t)n * Q * LEAD_STATS * sizeof(float)) + 255) & ~(size_t)255; }
static size_t lead_gemm_ws_bytes(int Q, int C, int H, int HT, int q_n, int c_n) {
  size_t m = 0;
  auto up = [&](size_t b) { if (b > m) m = b; };
  if (q_n > 0) { up(simx_gemm_f32_workspace_bytes(q_n, H, C)); up(simx_gemm_f32_workspace_bytes(q_n, HT, C)); }
  if (c_n > 0) { up(simx_gemm_f32_workspace_bytes(c_n, H, Q)); up(simx_gemm_f32_workspace_bytes(c_n, HT, Q)); }
  return m;
}

// the per-row statistics of the n slots, then the split-K workspace the backward products share
extern "C" size_t simx_lead_scores_workspace_bytes(int n, int Q, int C, int H, int HT, int q_n, int c_n) {
  if (n < 1 || Q < 1 || C < 1 || H < 1 || HT < 1) return 0;
  return lead_stats_bytes(n, Q) + lead_gemm_ws_bytes(Q, C, H, HT, q_n, c_n);
}

extern "C" int simx_lead_scores_fwd_bwd(simx_stream_t stream, int n, int Q, int C, int H, int HT, const float* q, const float* ctx,
                                        const float* tq, const float* tctx, const int32_t* pos_idx, float temperature,
                                        float layer_temperature, const simx_lead_slot* slots_host, int teacher_grad, float loss_scale,
                                        int q_lo, int q_n, int c_lo, int c_n, float* scores, float* tscores, float* slot_losses,
                                        float* weights, float* total, float* dq, float* dctx, float* dtq, float* dtctx, void* ws,
                                        size_t ws_bytes) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_REQUIRE(n >= 1 && n <= SIMX_LEAD_MAX_SLOTS, SIMX_ERR_BAD_SHAPE, "lead_scores: need 1 <= n=%d <= %d slots", n, SIMX_LEAD_MAX_SLOTS);
  SIMX_REQUIRE(Q > 0 && C > 0 && H > 0 && HT > 0, SIMX_ERR_BAD_SHAPE, "lead_scores: bad shape");
  SIMX_REQUIRE(temperature > 0.f, SIMX_ERR_BAD_SHAPE, "lead_scores: temperature must be > 0");
  SIMX_REQUIRE(slots_host != nullptr, SIMX_ERR_BAD_SHAPE, "lead_scores: slots are NULL");
  lead_slots sl = {};
  bool any_rw = false;
  for (int i = 0; i < n; ++i) { sl.s[i] = slots_host[i]; any_rw = any_rw || slots_host[i].reweight != 0; }
  SIMX_REQUIRE(!any_rw || layer_temperature > 0.f, SIMX_ERR_BAD_SHAPE, "lead_scores: layer_temperature must be > 0 with a reweight slot");
  SIMX_REQUIRE(q_lo >= 0 && q_n >= 0 && q_lo + q_n <= Q && c_lo >= 0 && c_n >= 0 && c_lo + c_n <= C, SIMX_ERR_BAD_SHAPE,
               "lead_scores: local slot out of range");
  SIMX_REQUIRE(q && ctx && tq && tctx && pos_idx && scores && tscores && slot_losses && weights && total, SIMX_ERR_BAD_SHAPE,
               "lead_scores: NULL argument");
  SIMX_REQUIRE((q_n == 0 || dq) && (c_n == 0 || dctx), SIMX_ERR_BAD_SHAPE, "lead_scores: NULL student gradient");
  SIMX_REQUIRE(!teacher_grad || ((q_n == 0 || dtq) && (c_n == 0 || dtctx)), SIMX_ERR_BAD_SHAPE, "lead_scores: NULL teacher gradient");
  const size_t need = simx_lead_scores_workspace_bytes(n, Q, C, H, HT, q_n, c_n);
  SIMX_REQUIRE(ws != nullptr && ws_bytes >= need, SIMX_ERR_WORKSPACE, "lead_scores: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);
  float* stats = reinterpret_cast<float*>(ws);
  const size_t gws_bytes = ws_bytes - lead_stats_bytes(n, Q);
  void* gws = gws_bytes ? reinterpret_cast<char*>(ws) + lead_stats_bytes(n, Q) : nullptr;
  const long QC = (long)Q * C;
  int rc;
  for (int i = 0; i < n; ++i) {                                                                // S_i = q_i ctx_i^T, Z_i = tq_i tctx_i^T
    rc = simx_gemm_f32_strided(stream, Q, C, H, q + (long)i * Q * H, H, 1, ctx + (long)i * C * H, 1, H, scores + i * QC, C, 0);
    if (rc) return rc;
    rc = simx_gemm_f32_strided(stream, Q, C, HT, tq + (long)i * Q * HT, HT, 1, tctx + (long)i * C * HT, 1, HT, tscores + i * QC, C, 0);
    if (rc) return rc;
  }
  const float ls = loss_scale == 0.f ? 1.f : loss_scale, iT = 1.0f / temperature;
  const dim3 grid(cdiv(Q, 4), n);
  hipLaunchKernelGGL(lead_row_stats_kernel, grid, dim3(256), 0, s, Q, C, scores, tscores, pos_idx, iT, stats);
  SIMX_CHECK_LAUNCH("lead_row_stats");
  hipLaunchKernelGGL(lead_reduce_kernel, dim3(1), dim3(256), 0, s, n, Q, stats, sl, any_rw ? 1.0f / layer_temperature : 0.f, ls,
                     slot_losses, weights, total);
  SIMX_CHECK_LAUNCH("lead_reduce");
  hipLaunchKernelGGL(lead_grad_kernel, grid, dim3(256), 0, s, Q, C, scores, tscores, pos_idx, iT, sl, weights, stats, ls / (float)Q,
                     teacher_grad);
  SIMX_CHECK_LAUNCH("lead_grad");
  for (int i = 0; i < n; ++i) {
    const float* dS = scores + i * QC;
    const float* dZ = tscores + i * QC;
    const float *qi = q + (long)i * Q * H, *ci = ctx + (long)i * C * H, *tqi = tq + (long)i * Q * HT, *tci = tctx + (long)i * C * HT;
    if (q_n > 0) {                                                                             // dQ_loc = dS[rows] ctx
      rc = simx_gemm_f32_strided_ws(stream, q_n, H, C, dS + (long)q_lo * C, C, 1, ci, H, 1, dq + (long)i * q_n * H, H, 0, gws, gws_bytes);
      if (rc) return rc;
      if (teacher_grad) {
        rc = simx_gemm_f32_strided_ws(stream, q_n, HT, C, dZ + (long)q_lo * C, C, 1, tci, HT, 1, dtq + (long)i * q_n * HT, HT, 0, gws, gws_bytes);
        if (rc) return rc;
      }
    }
    if (c_n > 0) {                                                                             // dC_loc = dS[:,cols]^T q
      rc = simx_gemm_f32_strided_ws(stream, c_n, H, Q, dS + c_lo, 1, C, qi, H, 1, dctx + (long)i * c_n * H, H, 0, gws, gws_bytes);
      if (rc) return rc;
      if (teacher_grad) {
        rc = simx_gemm_f32_strided_ws(stream, c_n, HT, Q, dZ + c_lo, 1, C, tqi, HT, 1, dtctx + (long)i * c_n * HT, HT, 0, gws, gws_bytes);
        if (rc) return rc;
      }
    }
  }
  return SIMX_OK;
}
