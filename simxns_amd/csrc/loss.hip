// Similarity + loss kernels (f32): wavefront-reduction kernels, one wave per query row.
//   sim_loss_kernel   : M1 einsum("bh,bdh->bd") + {L1 KL-distill, L2 NQ/TQ normal+adv, L3 CE+KD (every KD_type), L6 CE}
//                       forward AND closed-form backward in one launch -- replaces the
//                       5+ ATen launches and two .item() syncs of co_training_marco_train.py:199-224.
//   score_rows_kernel : M2 log_softmax / nll_loss / argmax over the all-pairs score matrix (SimANS/model/models.py:468-505),
//                       L4 the same rows with the KD_type objectives of BiEncoderKDLoss against the teacher's all-pairs scores,
//                       and dS in place: one body, one instantiation per objective.  bi_logit_rows_kernel is L4's Bi_logit
//                       objective, an MSE on the embeddings themselves.
//   scores_fwd_bwd    : the host side of every all-pairs entry point (score products, launch, backward products).
#include "common.h"
#include "prof.h"

#define LOSS_EPS 1e-7f

// the four loss scalars of one row: f32 atomics, or (SIMX_DETERMINISTIC=1) row `row` of a [rows][4] partial buffer that
// det_reduce_kernel adds in row order
__device__ __forceinline__ void loss_row_out(float* losses, float* det_part, int row, float l0, float l1, float l2, float l3) {
  if (det_part) {
    *reinterpret_cast<float4*>(det_part + 4L * row) = make_float4(l0, l1, l2, l3);
  } else {
    atomicAdd(losses + 0, l0);
    if (l1 != 0.f) atomicAdd(losses + 1, l1);
    if (l2 != 0.f) atomicAdd(losses + 2, l2);
    atomicAdd(losses + 3, l3);
  }
}
static int loss_det_begin(hipStream_t s, int rows, float** part) {
  *part = nullptr;
  if (!simx_det()) return SIMX_OK;
  *part = simx_det_ws(s, (size_t)rows * 4 * sizeof(float));
  return *part ? SIMX_OK : SIMX_ERR_WORKSPACE;
}

// softmax of x over the active lanes (0 on the others); mx / sum: the maximum and the sum of exp(x - mx), for log_softmax
__device__ __forceinline__ float wave_softmax(bool act, float x, float& mx, float& sum) {
  mx = wave_max(act ? x : -INFINITY);
  const float e = act ? expf(x - mx) : 0.f;
  sum = wave_sum(e);
  return e / sum;
}
__device__ __forceinline__ float wave_softmax(bool act, float x) {
  float mx, sum;
  return wave_softmax(act, x, mx, sum);
}

__global__ __launch_bounds__(256) void sim_loss_kernel(int B, int D, int H, const float* __restrict__ q,
                                                       const float* __restrict__ ctx, const float* __restrict__ teacher,
                                                       simx_loss_params lp, float* __restrict__ sim,
                                                       float* __restrict__ losses, float* __restrict__ dq,
                                                       float* __restrict__ dctx, float* __restrict__ det_part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const bool act = lane < D;
  // ---- similarity: lane d ends up holding s[b,d]
  float s = 0.f;
  if (q) {
    const float* qr = q + (long)b * H;
    for (int d = 0; d < D; ++d) {
      const float* cr = ctx + ((long)b * D + d) * H;
      float part = 0.f;
      for (int h = lane; h < H; h += 64) part = fmaf(qr[h], cr[h], part);
      part = wave_sum(part);
      if (lane == d) s = part;
    }
    if (act) sim[(long)b * D + lane] = s;
  } else if (act) {
    s = sim[(long)b * D + lane];
  }
  const float invB = 1.0f / (float)B;
  const float z = (act && teacher) ? teacher[(long)b * D + lane] : 0.f;
  float ds = 0.f, l0 = 0.f, l1 = 0.f, l2 = 0.f, corr = 0.f;
  // softmax of the (scaled) student logits
  const float ss = s * lp.scale;
  float ms, sums;
  const float p = wave_softmax(act, ss, ms, sums);
  if (lp.kind == SIMX_LOSS_KL || lp.kind == SIMX_LOSS_WIKI) {
    const float t = wave_softmax(act, z / lp.temperature);
    const float lp_eps = logf(p + LOSS_EPS);
    float g;
    if (lp.kind == SIMX_LOSS_KL) {
      const float term = (act && t > 0.f) ? t * (logf(t) - lp_eps) : 0.f;
      l1 = wave_sum(term) * invB;                                  // distill loss
      l0 = l1;
      g = -t * invB / (p + LOSS_EPS);
    } else {
      // reward = log(softmax([z0, zd])[0] + eps)
      const float z0 = __shfl(z, 0, 64);
      const float mx = fmaxf(z0, z);
      const float r = logf(expf(z0 - mx) / (expf(z0 - mx) + expf(z - mx)) + LOSS_EPS);
      l1 = wave_sum(act ? -t * lp_eps : 0.f) * invB;               // normal
      l2 = wave_sum(act ? r * lp_eps : 0.f);                       // adv (not / B)
      l0 = lp.adv_lambda * l2 + (1.0f - lp.adv_lambda) * l1;
      g = (lp.adv_lambda * r - (1.0f - lp.adv_lambda) * t * invB) / (p + LOSS_EPS);
    }
    const float gp = wave_sum(act ? g * p : 0.f);
    ds = act ? p * (g - gp) * lp.scale : 0.f;
  } else {
    // hard CE on target 0 (log_softmax of the raw logits; scale is 1 for these losses)
    const float lsm = ss - ms - logf(sums);
    const float hard = -__shfl(lsm, 0, 64) * invB;
    const float s0 = __shfl(ss, 0, 64);
    corr = (s0 >= ms) ? 1.f : 0.f;
    const float e0 = lane == 0 ? 1.f : 0.f;
    if (lp.kind == SIMX_LOSS_CE) {
      l0 = hard; l1 = hard;
      ds = act ? (p - e0) * invB : 0.f;
    } else if (lp.kind == SIMX_LOSS_CEKD) {
      const float Tm = lp.temperature;
      const float sT = s / Tm, zT = z / Tm;
      float m1, su1;
      const float pT = wave_softmax(act, sT, m1, su1), u = wave_softmax(act, zT);
      const float lpT = sT - m1 - logf(su1);
      const float term = (act && u > 0.f) ? u * (logf(u) - lpT) : 0.f;
      const float soft = wave_sum(term) * Tm * Tm * invB;
      l1 = hard; l2 = soft;
      l0 = lp.ce_w * hard + lp.kd_w * soft;
      ds = act ? lp.ce_w * (p - e0) * invB + lp.kd_w * (Tm * invB) * (pT - u) : 0.f;
    } else {
      // the other KD_type objectives of CrossBERTKDLoss: soft and dsoft = d soft / d s[b,lane]
      const float Tm = lp.temperature;
      float soft, dsoft;
      if (lp.kind == SIMX_LOSS_CE_LOGIT) {
        // KD_logit (:778-780): 0.5 * mean over all B*D elements of (s - z)^2
        const float inv = invB / (float)D;
        const float df = act ? s - z : 0.f;
        soft = 0.5f * wave_sum(df * df) * inv;
        dsoft = df * inv;
      } else {
        const float zT = z / Tm;
        const float u = wave_softmax(act, zT);                         // softmax(z / T)
        if (lp.kind == SIMX_LOSS_CE_PROB) {
          // prob_loss (:738-743): -(1/B) sum u log(softmax(s) + eps), the student without temperature
          const float lp_eps = logf(p + LOSS_EPS);
          soft = wave_sum(act ? -u * lp_eps : 0.f) * invB;
          const float g = -u * invB / (p + LOSS_EPS);
          const float gp = wave_sum(act ? g * p : 0.f);
          dsoft = act ? p * (g - gp) : 0.f;
        } else {
          // DKD (dkd_loss, :784-808), target column 0.  tckd: KL of the two-bin distributions {target, all others}, the
          // "others" bin a sum over the non-target lanes as cat_mask forms it; nckd: KL of the softmaxes with 1000 taken
          // off the target logit.
          const float sT = s / Tm;
          const float pT = wave_softmax(act, sT);
          const bool oth = act && lane != 0;
          const float p_gt = __shfl(pT, 0, 64), u_gt = __shfl(u, 0, 64);
          const float p_o = wave_sum(oth ? pT : 0.f), u_o = wave_sum(oth ? u : 0.f);
          float tckd = 0.f;
          if (u_gt > 0.f) tckd += u_gt * (logf(u_gt) - logf(p_gt));
          if (u_o > 0.f) tckd += u_o * (logf(u_o) - logf(p_o));
          const float sm = sT - 1000.0f * e0, zm = zT - 1000.0f * e0;
          float m3, su3;
          const float pm = wave_softmax(act, sm, m3, su3), um = wave_softmax(act, zm);
          const float lpm = sm - m3 - logf(su3);
          const float nckd = wave_sum((act && um > 0.f) ? um * (logf(um) - lpm) : 0.f);
          soft = (lp.dkd_alpha * tckd + lp.dkd_beta * nckd) * Tm * Tm * invB;
          const float tc = lane == 0 ? pT - u : pT * (p_o - u_o) / p_o;
          dsoft = act ? (Tm * invB) * (lp.dkd_alpha * tc + lp.dkd_beta * (pm - um)) : 0.f;
        }
      }
      l1 = hard; l2 = soft;
      l0 = lp.ce_w * hard + lp.kd_w * soft;
      ds = act ? lp.ce_w * (p - e0) * invB + lp.kd_w * dsoft : 0.f;
    }
  }
  const float ga = 1.0f / lp.grad_accum;
  ds *= ga;
  if (lane == 0) loss_row_out(losses, det_part, b, l0 * ga, l1, l2, corr);
  // ---- backward of the similarity
  if (q) {
    const float* qr = q + (long)b * H;
    for (int h = lane; h < H; h += 64) {
      float acc = 0.f;
      const float qv = qr[h];
      for (int d = 0; d < D; ++d) {
        const float dsd = __shfl(ds, d, 64);
        const long o = ((long)b * D + d) * H + h;
        acc = fmaf(dsd, ctx[o], acc);
        dctx[o] = dsd * qv;
      }
      dq[(long)b * H + h] = acc;
    }
  } else if (act) {
    dctx[(long)b * D + lane] = ds;
  }
}

// All-pairs rows (M2 / L4), one wave per row of the student scores S [Q,C]; KD picks the objective: KD_NONE (BiEncoderNllLoss,
// no teacher) or the SIMX_KD_* types of BiEncoderKDLoss against the teacher scores Z [Q,C].  Per row
//   hard = NLL(log_softmax(S), pos), correct = (argmax S == pos, first index on ties: torch.max semantics), and soft:
//   SIMX_KD_SOFTMAX   T^2 sum_c u (log u - log_softmax(S/T)), u = softmax(Z/T)                   (kd_loss, :772-781)
//   SIMX_KD_LOGIT     0.5 * sum_c (S - Z)^2 / C                                                   (kd_loss KD_logit, :1056-1058)
//   SIMX_KD_DKD       T^2 (alpha tckd + beta nckd), target column pos                             (dkd_loss, :1070-1094)
//   SIMX_KD_BI_LOGIT  0 here: the hard term only, Z is not read (bi_logit_rows_kernel adds the embedding MSE)
// then S <- dS in place: KD_NONE (softmax(S) - onehot) * gscale, loss (hard * lscale / Q, 0, 0, correct) and the optional
// row_stats[2i] = max, [2i+1] = lse; the others gscale * (ce_w (softmax(S) - onehot) + kd_w dsoft/dS), loss
// ((ce_w hard + kd_w soft) * lscale, hard, soft) / Q.  What looks alike across the objectives does not always round alike
// (the teacher's max and sum of KD_softmax and DKD, (kd_w T) (pT - u) against kd_w (T ...)): each keeps its own order of
// operations inside its `if constexpr`, and only what is bit-for-bit common is written once.
constexpr int KD_NONE = -1;
template <int KD>
__global__ __launch_bounds__(256) void score_rows_kernel(int Q, int C, float* __restrict__ scores, const float* __restrict__ tscores,
                                                         const int* __restrict__ pos_idx, float T, float ce_w, float kd_w,
                                                         float alpha, float beta, float gscale, float lscale,
                                                         float* __restrict__ row_stats, float* __restrict__ losses,
                                                         float* __restrict__ det_part) {
  constexpr bool SM = KD == SIMX_KD_SOFTMAX, LOGIT = KD == SIMX_KD_LOGIT, DKD = KD == SIMX_KD_DKD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w;
  if (i >= Q) return;
  float* r = scores + (long)i * C;
  const float* z = (SM || LOGIT || DKD) ? tscores + (long)i * C : nullptr;
  const int pos = pos_idx[i];
  const float iT = 1.0f / T;
  // maxima: of S (with its arg-max); KD_softmax of Z; DKD of Z/T, and of S/T and Z/T with 1000 taken off the target column
  float m = -INFINITY, mz = -INFINITY, mm = -INFINITY, mzm = -INFINITY;
  int am = 0x7FFFFFFF;
  for (int c = lane; c < C; c += 64) {
    const float v = r[c];
    if (v > m) { m = v; am = c; }
    if constexpr (SM) mz = fmaxf(mz, z[c]);
    if constexpr (DKD) {
      const float zc = z[c] * iT, off = c == pos ? 1000.0f : 0.f;
      mz = fmaxf(mz, zc);
      mm = fmaxf(mm, v * iT - off);
      mzm = fmaxf(mzm, zc - off);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  if constexpr (SM || DKD) mz = wave_max(mz);
  if constexpr (DKD) { mm = wave_max(mm); mzm = wave_max(mzm); }
  // sums: s1 of exp(S - m); KD_softmax and DKD of the S/T and Z/T terms (sz: each its own form of the same softmax(Z/T))
  float s1 = 0.f, sT = 0.f, sTo = 0.f, sz = 0.f, szo = 0.f, sm = 0.f, szm = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = r[c];
    s1 += expf(v - m);
    if constexpr (SM) {
      sT += expf((v - m) * iT);
      sz += expf((z[c] - mz) * iT);
    }
    if constexpr (DKD) {
      const bool gt = c == pos;
      const float zc = z[c] * iT, off = gt ? 1000.0f : 0.f;
      const float eT = expf((v - m) * iT), eZ = expf(zc - mz);
      sT += eT; sz += eZ;
      if (!gt) { sTo += eT; szo += eZ; }                // the "others" bin of cat_mask: a sum of the non-target terms
      sm += expf(v * iT - off - mm);
      szm += expf(zc - off - mzm);
    }
  }
  s1 = wave_sum(s1);
  const float lse = m + logf(s1);
  const float sp = r[pos];
  float lseT = 0.f, lseZ = 0.f, lseM = 0.f, lseZM = 0.f, u_gt = 0.f, ko = 0.f, tckd = 0.f;
  if constexpr (SM || DKD) { sT = wave_sum(sT); sz = wave_sum(sz); lseT = m * iT + logf(sT); }
  if constexpr (SM) lseZ = mz * iT + logf(sz);
  if constexpr (DKD) {
    sTo = wave_sum(sTo); szo = wave_sum(szo); sm = wave_sum(sm); szm = wave_sum(szm);
    lseM = mm + logf(sm); lseZM = mzm + logf(szm);
    const float p_gt = expf(sp * iT - lseT), p_o = sTo / sT, u_o = szo / sz;
    u_gt = expf(z[pos] * iT - (mz + logf(sz)));
    if (u_gt > 0.f) tckd += u_gt * (logf(u_gt) - logf(p_gt));
    if (u_o > 0.f) tckd += u_o * (logf(u_o) - logf(p_o));
    ko = (p_o - u_o) / p_o;
  }
  if constexpr (KD == KD_NONE) {
    if (row_stats && lane == 0) { row_stats[2 * i] = m; row_stats[2 * i + 1] = lse; }
  }
  float soft = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = r[c];
    const bool gt = c == pos;
    const float p1 = expf(v - lse), hot = gt ? 1.f : 0.f;
    float g;                                            // dS[i,c]
    if constexpr (KD == KD_NONE) {
      g = (p1 - hot) * gscale;
    } else if constexpr (SM) {
      const float lu = z[c] * iT - lseZ;                // log u
      const float u = expf(lu);
      const float lpT = v * iT - lseT;                  // log_softmax(S/T)
      if (u > 0.f) soft += u * (lu - lpT);
      const float pT = expf(lpT);
      g = gscale * (ce_w * (p1 - hot) + kd_w * T * (pT - u));
    } else {
      float d = 0.f;                                    // d soft / d S[i,c]
      if constexpr (LOGIT) {
        const float df = v - z[c];
        soft = fmaf(df, df, soft);
        d = df / (float)C;
      }
      if constexpr (DKD) {
        const float off = gt ? 1000.0f : 0.f;
        const float pT = expf(v * iT - lseT);
        const float lpm = v * iT - off - lseM, lum = z[c] * iT - off - lseZM;
        const float um = expf(lum);
        if (um > 0.f) soft += um * (lum - lpm);
        d = T * (alpha * (gt ? pT - u_gt : pT * ko) + beta * (expf(lpm) - um));
      }
      g = gscale * (ce_w * (p1 - hot) + kd_w * d);
    }
    r[c] = g;
  }
  if constexpr (KD != KD_NONE) soft = wave_sum(soft);
  if constexpr (SM) soft = soft * T * T;
  if constexpr (LOGIT) soft *= 0.5f / (float)C;
  if constexpr (DKD) soft = (alpha * tckd + beta * soft) * T * T;
  if (lane == 0) {
    const float hard = lse - sp;
    float l0, l1 = 0.f, l2 = 0.f;
    if constexpr (KD == KD_NONE) {
      l0 = hard * lscale / (float)Q;
    } else {
      l0 = (ce_w * hard + kd_w * soft) * lscale / (float)Q; l1 = hard / (float)Q; l2 = soft / (float)Q;
    }
    loss_row_out(losses, det_part, i, l0, l1, l2, am == pos ? 1.f : 0.f);
  }
}

// Bi_logit (bi_logit, :1062-1067): 0.5 * MSE(q, tq) + 0.5 * MSE(ctx, tctx) on the gathered embeddings, one wave per row
// (rows [0,Q) = q, [Q,Q+C) = ctx).  Every row counts in the loss; only the local rows get kd_w * lscale * (x - t) / (rows * H)
// added to the gradient the score products left in dq_local / dctx_local.
__global__ __launch_bounds__(256) void bi_logit_rows_kernel(int Q, int C, int H, const float* __restrict__ q, const float* __restrict__ ctx,
                                                            const float* __restrict__ tq, const float* __restrict__ tctx, float kd_w,
                                                            float lscale, int q_lo, int q_n, int c_lo, int c_n,
                                                            float* __restrict__ dq_local, float* __restrict__ dctx_local,
                                                            float* __restrict__ losses, float* __restrict__ det_part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w;
  if (i >= Q + C) return;
  const bool isq = i < Q;
  const int row = isq ? i : i - Q, rows = isq ? Q : C;
  const int lo = isq ? q_lo : c_lo, n = isq ? q_n : c_n;
  const float* x = (isq ? q : ctx) + (long)row * H;
  const float* t = (isq ? tq : tctx) + (long)row * H;
  float* d = isq ? dq_local : dctx_local;
  const bool local = d != nullptr && row >= lo && row < lo + n;
  if (local) d += (long)(row - lo) * H;
  const float inv = 1.0f / ((float)rows * (float)H);
  const float gw = kd_w * lscale * inv;
  float acc = 0.f;
  for (int h = lane; h < H; h += 64) {
    const float df = x[h] - t[h];
    acc = fmaf(df, df, acc);
    if (local) d[h] += gw * df;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const float soft = 0.5f * acc * inv;
    loss_row_out(losses, det_part, i, kd_w * lscale * soft, 0.f, soft, 0.f);
  }
}

// split-K workspace of the two backward products (dQ_loc: [q_n,H] over K = C; dC_loc: [c_n,H] over K = Q)
extern "C" size_t simx_scores_workspace_bytes(int Q, int C, int H, int q_n, int c_n) {
  const size_t a = q_n > 0 ? simx_gemm_f32_workspace_bytes(q_n, H, C) : 0, b = c_n > 0 ? simx_gemm_f32_workspace_bytes(c_n, H, Q) : 0;
  return a > b ? a : b;
}

extern "C" int simx_sim_loss_fwd_bwd(simx_stream_t stream, int B, int D, int H, const float* q, const float* ctx,
                                     const float* teacher, const simx_loss_params* lp, float* sim, float* losses,
                                     float* dq, float* dctx) {
  hipStream_t s = (hipStream_t)stream;
  SIMX_PROF(SIMX_K_LOSS, s, 16.0 * B * D * (H > 0 ? H : 1));
  SIMX_REQUIRE(lp != nullptr, SIMX_ERR_BAD_SHAPE, "sim_loss: params are NULL");
  SIMX_REQUIRE(B > 0 && D > 0 && D <= 64, SIMX_ERR_UNSUPPORTED, "sim_loss: need 0 < D=%d <= 64", D);
  SIMX_REQUIRE(lp->kind >= 0 && lp->kind <= SIMX_LOSS_CE_PROB, SIMX_ERR_UNSUPPORTED, "sim_loss: kind %d", lp->kind);
  SIMX_REQUIRE(lp->kind == SIMX_LOSS_CE || teacher != nullptr, SIMX_ERR_BAD_SHAPE, "sim_loss: teacher logits missing");
  SIMX_REQUIRE(q == nullptr || (ctx && dq && H > 0), SIMX_ERR_BAD_SHAPE, "sim_loss: q given without ctx/dq");
  SIMX_REQUIRE(sim && losses && dctx, SIMX_ERR_BAD_SHAPE, "sim_loss: NULL output");
  SIMX_REQUIRE(lp->grad_accum > 0.f && lp->temperature != 0.f, SIMX_ERR_BAD_SHAPE, "sim_loss: bad grad_accum/temperature");
  if (hipMemsetAsync(losses, 0, 4 * sizeof(float), s) != hipSuccess) { simx_set_error("sim_loss: memset failed"); return SIMX_ERR_HIP; }
  float* det = nullptr;
  if (int rcd = loss_det_begin(s, B, &det)) return rcd;
  hipLaunchKernelGGL(sim_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, B, D, H, q, ctx, teacher, *lp, sim, losses, dq, dctx, det);
  SIMX_CHECK_LAUNCH("sim_loss");
  if (det) return simx_det_reduce(s, det, 4L, B, 4, losses, nullptr, nullptr, nullptr);
  return SIMX_OK;
}

// The all-pairs losses on the host: S = q ctx^T (and Z = tq tctx^T), the row kernel of `kd`, the ordered reduction of
// SIMX_DETERMINISTIC=1, the two backward products on the local slots and Bi_logit's embedding MSE.  kd == KD_NONE is the NLL
// entry, which checks neither the teacher's arguments nor for NULL; `who` names the entry in the error text.
static int scores_fwd_bwd(const char* who, simx_stream_t stream, int kd, int Q, int C, int H, int HT, const float* q, const float* ctx,
                          const float* tq, const float* tctx, const int32_t* pos_idx, float temperature, float ce_w, float kd_w,
                          float dkd_alpha, float dkd_beta, float loss_scale, int q_lo, int q_n, int c_lo, int c_n, float* scores,
                          float* tscores, float* row_stats, float* losses, float* dq_local, float* dctx_local, void* ws,
                          size_t ws_bytes) {
  hipStream_t s = (hipStream_t)stream;
  const bool kdf = kd != KD_NONE, bi = kd == SIMX_KD_BI_LOGIT;
  auto rows = kd == KD_NONE            ? score_rows_kernel<KD_NONE>
              : kd == SIMX_KD_SOFTMAX  ? score_rows_kernel<SIMX_KD_SOFTMAX>
              : kd == SIMX_KD_LOGIT    ? score_rows_kernel<SIMX_KD_LOGIT>
              : kd == SIMX_KD_DKD      ? score_rows_kernel<SIMX_KD_DKD>
              : kd == SIMX_KD_BI_LOGIT ? score_rows_kernel<SIMX_KD_BI_LOGIT>
                                       : nullptr;
  SIMX_REQUIRE(rows != nullptr, SIMX_ERR_UNSUPPORTED, "%s: kd_type %d", who, kd);
  SIMX_REQUIRE(Q > 0 && C > 0 && H > 0 && (!kdf || HT > 0), SIMX_ERR_BAD_SHAPE, "%s: bad shape", who);
  SIMX_REQUIRE(!bi || H == HT, SIMX_ERR_BAD_SHAPE, "%s: Bi_logit compares embeddings, teacher width %d != student width %d", who, HT, H);
  SIMX_REQUIRE(!kdf || temperature > 0.f, SIMX_ERR_BAD_SHAPE, "%s: temperature must be > 0", who);
  SIMX_REQUIRE(q_lo >= 0 && q_n >= 0 && q_lo + q_n <= Q && c_lo >= 0 && c_n >= 0 && c_lo + c_n <= C, SIMX_ERR_BAD_SHAPE,
               "%s: local slot out of range", who);
  SIMX_REQUIRE(!kdf || (q && ctx && tq && tctx && pos_idx && scores && (tscores || bi) && losses), SIMX_ERR_BAD_SHAPE,
               "%s: NULL argument", who);
  if (hipMemsetAsync(losses, 0, 4 * sizeof(float), s) != hipSuccess) { simx_set_error("%s: memset failed", who); return SIMX_ERR_HIP; }
  int rc = simx_gemm_f32_strided(stream, Q, C, H, q, H, 1, ctx, 1, H, scores, C, 0);          // S = q ctx^T
  if (rc) return rc;
  if (kdf && !bi) {
    rc = simx_gemm_f32_strided(stream, Q, C, HT, tq, HT, 1, tctx, 1, HT, tscores, C, 0);      // Z = tq tctx^T
    if (rc) return rc;
  }
  const float ls = loss_scale == 0.f ? 1.f : loss_scale;
  float* det = nullptr;
  if (int rcd = loss_det_begin(s, Q, &det)) return rcd;
  hipLaunchKernelGGL(rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, Q, C, scores, tscores, pos_idx, temperature, ce_w, kd_w, dkd_alpha,
                     dkd_beta, ls / (float)Q, ls, row_stats, losses, det);
  SIMX_CHECK_LAUNCH("score_rows");
  if (det) { rc = simx_det_reduce(s, det, 4L, Q, 4, losses, nullptr, nullptr, nullptr); if (rc) return rc; }
  if (q_n > 0 && dq_local) {                                                                  // dQ_loc = dS[rows] ctx
    rc = simx_gemm_f32_strided_ws(stream, q_n, H, C, scores + (long)q_lo * C, C, 1, ctx, H, 1, dq_local, H, 0, ws, ws_bytes);
    if (rc) return rc;
  }
  if (c_n > 0 && dctx_local) {                                                                // dC_loc = dS[:,cols]^T q
    rc = simx_gemm_f32_strided_ws(stream, c_n, H, Q, scores + c_lo, 1, C, q, H, 1, dctx_local, H, 0, ws, ws_bytes);
    if (rc) return rc;
  }
  if (bi) {                                                                                   // + kd_w * embedding MSE, after the products
    if (int rcd = loss_det_begin(s, Q + C, &det)) return rcd;
    hipLaunchKernelGGL(bi_logit_rows_kernel, dim3(cdiv(Q + C, 4)), dim3(256), 0, s, Q, C, H, q, ctx, tq, tctx, kd_w, ls, q_lo, q_n, c_lo,
                       c_n, dq_local, dctx_local, losses, det);
    SIMX_CHECK_LAUNCH("bi_logit_rows");
    if (det) return simx_det_reduce(s, det, 4L, Q + C, 4, losses, nullptr, nullptr, nullptr);
  }
  return SIMX_OK;
}

extern "C" int simx_scores_nll_fwd_bwd(simx_stream_t stream, int Q, int C, int H, const float* q, const float* ctx,
                                       const int32_t* pos_idx, float loss_scale, int q_lo, int q_n, int c_lo, int c_n,
                                       float* scores, float* row_stats, float* losses, float* dq_local, float* dctx_local,
                                       void* ws, size_t ws_bytes) {
  return scores_fwd_bwd("scores_nll", stream, KD_NONE, Q, C, H, 0, q, ctx, nullptr, nullptr, pos_idx, 1.f, 0.f, 0.f, 0.f, 0.f, loss_scale,
                        q_lo, q_n, c_lo, c_n, scores, nullptr, row_stats, losses, dq_local, dctx_local, ws, ws_bytes);
}

extern "C" int simx_scores_kd_type_fwd_bwd(simx_stream_t stream, int kd_type, int Q, int C, int H, int HT, const float* q,
                                           const float* ctx, const float* tq, const float* tctx, const int32_t* pos_idx,
                                           float temperature, float ce_w, float kd_w, float dkd_alpha, float dkd_beta,
                                           float loss_scale, int q_lo, int q_n, int c_lo, int c_n, float* scores, float* tscores,
                                           float* losses, float* dq_local, float* dctx_local, void* ws, size_t ws_bytes) {
  SIMX_REQUIRE(kd_type != KD_NONE, SIMX_ERR_UNSUPPORTED, "scores_kd: kd_type %d", kd_type);   // unit-local, not a kd_type of the interface
  return scores_fwd_bwd("scores_kd", stream, kd_type, Q, C, H, HT, q, ctx, tq, tctx, pos_idx, temperature, ce_w, kd_w, dkd_alpha, dkd_beta,
                        loss_scale, q_lo, q_n, c_lo, c_n, scores, tscores, nullptr, losses, dq_local, dctx_local, ws, ws_bytes);
}

extern "C" int simx_scores_kd_fwd_bwd(simx_stream_t stream, int Q, int C, int H, int HT, const float* q, const float* ctx,
                                      const float* tq, const float* tctx, const int32_t* pos_idx, float temperature,
                                      float ce_w, float kd_w, float loss_scale, int q_lo, int q_n, int c_lo, int c_n,
                                      float* scores, float* tscores, float* losses, float* dq_local, float* dctx_local,
                                      void* ws, size_t ws_bytes) {
  return simx_scores_kd_type_fwd_bwd(stream, SIMX_KD_SOFTMAX, Q, C, H, HT, q, ctx, tq, tctx, pos_idx, temperature, ce_w, kd_w, 0.f, 0.f,
                                     loss_scale, q_lo, q_n, c_lo, c_n, scores, tscores, losses, dq_local, dctx_local, ws, ws_bytes);
}
