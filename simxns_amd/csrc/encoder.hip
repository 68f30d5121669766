// The whole-encoder forward / backward driver.
// Sequences the gfx950 kernels for HFBertEncoder.forward (SimANS/model/models.py:77-82 -> HF
// BertModel.forward, spec LEAD/modeling_bert.py:916-1038) and its backward on the packed token
// layout.  No allocation, no synchronisation: every buffer is carved from caller-provided memory.
//
// HBM layout (all 256-B aligned; each buffer is described once, by its walk_* function below):
//   params / grads : one f32 buffer each, canonical order (simx_bert_param_offset)
//   wcache         : per layer  Wqkv, Wqkv^T, Wo, Wo^T, W1, W1^T, W2, W2^T   (bf16 / fp16; f32 mode keeps only
//                    the transposes, in f32) -- rebuilt once per optimiser step                       (walk_wlayer)
//   act            : x0 | layer slots | the [CLS]-only last layer's compact tensors                   (walk_act)
//   bwd scratch    : bufA[T,H] bufB[T,H] bufC[T,H] du[T,F] dqkv[T,3H] | split-K slabs of the wgrad GEMMs | ...   (walk_scratch)
#include "common.h"

// ------------------------------------------------------------------------------------------ layouts
static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t esz(int dtype) { return dtype == SIMX_F32 ? 4 : 2; }

static bool cfg_ok(const simx_bert_cfg* c) {
  return c && simx_dtype_ok(c->dtype) && c->qkv_layout >= 0 && c->qkv_layout <= 1 && c->f32_gemm >= 0 && c->f32_gemm <= 1 && c->stream_lo >= 0 && c->stream_lo <= 1 && c->layers > 0 && c->hidden > 0 && c->heads > 0 &&
         c->hidden % c->heads == 0 && c->hidden % 4 == 0 && c->inter > 0 && c->inter % 4 == 0 && c->vocab > 0 &&
         c->max_pos > 0 && c->type_vocab > 0 && c->hidden <= 1024;
}

static size_t layer_param_count(const simx_bert_cfg* c) {
  const size_t H = c->hidden, F = c->inter;
  return 3 * H * H + 3 * H + H * H + H + 2 * H + F * H + F + H * F + H + 2 * H;
}

extern "C" size_t simx_bert_param_count(const simx_bert_cfg* c) {
  if (!cfg_ok(c)) return 0;
  const size_t H = c->hidden;
  return (size_t)c->vocab * H + (size_t)c->max_pos * H + (size_t)c->type_vocab * H + 2 * H +
         (size_t)c->layers * layer_param_count(c) + H * H + H;
}

extern "C" size_t simx_bert_param_offset(const simx_bert_cfg* c, int layer, int which) {
  if (!cfg_ok(c)) return (size_t)-1;
  const size_t H = c->hidden, F = c->inter;
  const size_t emb = (size_t)c->vocab * H + (size_t)c->max_pos * H + (size_t)c->type_vocab * H + 2 * H;
  if (layer == -1) {
    switch (which) {
      case SIMX_P_WORD: return 0;
      case SIMX_P_POS: return (size_t)c->vocab * H;
      case SIMX_P_TYPE: return (size_t)c->vocab * H + (size_t)c->max_pos * H;
      case SIMX_P_EMB_LN_G: return emb - 2 * H;
      case SIMX_P_EMB_LN_B: return emb - H;
      default: return (size_t)-1;
    }
  }
  if (layer >= 0 && layer < c->layers) {
    size_t o = emb + (size_t)layer * layer_param_count(c);
    const size_t sizes[12] = {3 * H * H, 3 * H, H * H, H, H, H, F * H, F, H * F, H, H, H};
    if (which < SIMX_P_WQKV || which > SIMX_P_LN2_B) return (size_t)-1;
    for (int i = 0; i < which - SIMX_P_WQKV; ++i) o += sizes[i];
    return o;
  }
  if (layer == c->layers) {
    const size_t o = emb + (size_t)c->layers * layer_param_count(c);
    if (which == SIMX_P_POOL_W) return o;
    if (which == SIMX_P_POOL_B) return o + H * H;
  }
  return (size_t)-1;
}

// "Operand planes" (csrc/gemm_xp.hip, simx.h): the fp32 engine's large towers run their dense GEMMs on pre-split 16-bit plane
// pairs.  Three predicates, each a function of its arguments only so that sizing calls, forward and backward agree:
//   pl_weights(c)            the weight cache also holds fp16 planes of W and bf16 planes of W^T
//   pl_layout(c, Tp)         activation / scratch buffers have room for the planes of the residual stream (x0, x1, xout)
//   pl_run(c, Tp, max_len)   the tower's full layers run on planes (needs the f32 MFMA attention: head size 64, sequences <= 4096)
// SIMX_F32_PLANES=0 pins the register-split kernels of gemm_x3.hip (A/B measurements); SIMX_F32_PLANES_MIN_TILES lowers the
// size threshold (tests run small towers through the plane kernels).
static bool pl_weights(const simx_bert_cfg* c) {
  static const bool on = [] { const char* e = getenv("SIMX_F32_PLANES"); return !e || e[0] != '0'; }();
  return on && c->dtype == SIMX_F32 && c->f32_gemm == 0 && c->hidden % 256 == 0 && c->inter % 256 == 0 && c->hidden / c->heads == 64;
}
static bool pl_layout(const simx_bert_cfg* c, size_t Tp) {
  static const long min_tiles = [] { const char* e = getenv("SIMX_F32_PLANES_MIN_TILES"); return e ? atol(e) : 192L; }();
  return pl_weights(c) && (long)(Tp / 256) * (c->hidden / 256) >= min_tiles;
}
static bool pl_run(const simx_bert_cfg* c, size_t Tp, int max_len) { return pl_layout(c, Tp) && simx_mha_planes_ok(c->hidden / c->heads, max_len); }

// Bump carver.  Every caller-provided buffer is described ONCE, by the walk_* function that carves it with one of these and
// fills a struct of pointers.  A walk from a NULL base yields no pointers and leaves the buffer's size in `off`: the
// simx_bert_*_bytes entry points and the drivers run the same walk, so a size and a pointer chain cannot drift apart.
struct Carver {
  char* base;
  size_t off;
  char* at(size_t o) const { return base ? base + o : nullptr; }
  char* take(size_t bytes) { char* p = at(off); off += al(bytes); return p; }
  // the element walked since offset `first` is the first of n equal ones: skips the others, returns the stride
  size_t repeat(size_t first, size_t n) { const size_t stride = off - first; off = first + n * stride; return stride; }
};

// wqkvP .. w2P: fp16 plane pairs of W [out, in] (forward operand); wqkvTP .. w2TP: bf16 plane pairs of W^T [in, out] (dgrad)
struct WLayer { const char *wqkv, *wqkvT, *wo, *woT, *w1, *w1T, *w2, *w2T, *wqkvP, *woP, *w1P, *w2P, *wqkvTP, *woTP, *w1TP, *w2TP; };
static WLayer walk_wlayer(const simx_bert_cfg* c, Carver& k) {
  const size_t H = c->hidden, F = c->inter, e = esz(c->dtype);
  const size_t qkv = 3 * H * H * e, o = H * H * e, f = F * H * e;
  WLayer w = {};
  if (c->dtype == SIMX_F32) {                     // W itself is read from params (wlayer): the f32 transposes ...
    w.wqkvT = k.take(qkv); w.woT = k.take(o); w.w1T = k.take(f); w.w2T = k.take(f);
    if (pl_weights(c)) {                          // ... | fp16 planes of W | bf16 planes of W^T (4 B per element each)
      w.wqkvP = k.take(qkv); w.woP = k.take(o); w.w1P = k.take(f); w.w2P = k.take(f);
      w.wqkvTP = k.take(qkv); w.woTP = k.take(o); w.w1TP = k.take(f); w.w2TP = k.take(f);
    }
  } else {
    w.wqkv = k.take(qkv); w.wqkvT = k.take(qkv);
    w.wo = k.take(o); w.woT = k.take(o);
    w.w1 = k.take(f); w.w1T = k.take(f);
    w.w2 = k.take(f); w.w2T = k.take(f);
  }
  return w;
}
extern "C" size_t simx_bert_wcache_bytes(const simx_bert_cfg* c) {
  if (!cfg_ok(c)) return 0;
  Carver k{nullptr, 0};
  walk_wlayer(c, k);
  k.repeat(0, (size_t)c->layers);
  return k.off;
}
static WLayer wlayer(const simx_bert_cfg* c, const float* params, const void* wcache, int l) {
  Carver k{nullptr, 0};
  walk_wlayer(c, k);
  k = Carver{(char*)const_cast<void*>(wcache), (size_t)l * k.off};
  WLayer w = walk_wlayer(c, k);
  if (c->dtype == SIMX_F32) {
    w.wqkv = (const char*)(params + simx_bert_param_offset(c, l, SIMX_P_WQKV));
    w.wo = (const char*)(params + simx_bert_param_offset(c, l, SIMX_P_WO));
    w.w1 = (const char*)(params + simx_bert_param_offset(c, l, SIMX_P_W1));
    w.w2 = (const char*)(params + simx_bert_param_offset(c, l, SIMX_P_W2));
  }
  return w;
}

// Every token-major buffer is carved with its row count rounded up to a multiple of 256, and the NT GEMMs run on the
// padded row count: the persistent full-tile kernels then also serve ragged (packed, variable-length) batches.  Rows
// [T, Tp) hold garbage that never leaves its own row (an NT GEMM row depends on that row of A only; LayerNorm,
// attention, the wgrad contraction and every reduction run over the T real rows).
static inline int rows_cap(int T) { return (T + 255) & ~255; }
// stream_lo (simx.h): the residual stream -- x0 and every LayerNorm output -- is a 16-bit tensor PLUS a one-byte correction
// per element (x1l / xoutl, NULL otherwise); z1 / z2 then hold the dense outputs without the residual, which the LayerNorm
// kernels add
static inline bool stream_lo(const simx_bert_cfg* c) { return c->stream_lo != 0 && simx_is16(c->dtype); }
// a [Tp,H] tensor of the residual stream: the values, followed by the corrections (ONE BYTE per element: common.h lo8) when
// stream_lo, or by the fp16 plane pair of the f32 values with pl_layout (the two never coincide: 16-bit vs f32 towers)
struct XS { char *hi, *lo, *planes; };
static XS walk_xs(const simx_bert_cfg* c, Carver& k, size_t Tp) {
  XS x;
  x.hi = k.take(Tp * c->hidden * esz(c->dtype));
  x.lo = stream_lo(c) ? k.take(Tp * c->hidden) : nullptr;
  x.planes = pl_layout(c, Tp) ? k.take(Tp * c->hidden * 4) : nullptr;
  return x;
}
// x1p / xoutp (operand planes, pl_layout): the fp16 plane pairs of x1 / xout beside their f32 forms; in a layer that RUNS on planes
// the ctx and h slots hold plane pairs instead of f32 (same bytes: two 16-bit planes)
struct ALayer { char *qkv, *ctx, *z1, *x1, *u, *h, *z2, *xout, *x1l, *xoutl, *x1p, *xoutp; float* lse; };
static ALayer walk_alayer(const simx_bert_cfg* c, Carver& k, size_t T) {
  const size_t H = c->hidden, F = c->inter, e = esz(c->dtype);
  ALayer a;
  a.qkv = k.take(T * 3 * H * e);
  a.ctx = k.take(T * H * e);
  a.z1 = k.take(T * H * e);
  a.x1 = k.take(T * H * e);
  a.z2 = k.take(T * H * e);
  a.xout = k.take(T * H * e);
  a.x1l = a.xoutl = a.x1p = a.xoutp = nullptr;
  if (stream_lo(c)) { a.x1l = k.take(T * H); a.xoutl = k.take(T * H); }
  if (pl_layout(c, T)) { a.x1p = k.take(T * H * 4); a.xoutp = k.take(T * H * 4); }
  a.u = k.take(T * F * e);                     // gelu'(u) of the FFN pre-activation (SIMX_EPI_GELU writes it; only DGELU reads it)
  a.h = k.take(T * F * e);
  a.lse = (float*)k.take((size_t)c->heads * T * 4);
  return a;
}
// The [CLS]-only last layer's compact [n,H] tensors: q and the attention context of the [CLS] rows (kept for backward), a
// temporary, and -- stream_lo -- the gathered residual rows of the layer input with their correction bytes (kept for backward)
struct ClsExtra { char *qc, *ctxc, *ytmp, *xg, *xgl; };
static ClsExtra walk_cls_extra(const simx_bert_cfg* c, Carver& k, size_t n) {
  const size_t b = n * c->hidden * esz(c->dtype);
  ClsExtra x;
  x.qc = k.take(b);
  x.ctxc = k.take(b);
  x.ytmp = k.take(b);
  x.xg = k.take(b);
  x.xgl = k.take(b);
  return x;
}
// Activation memory, three modes:
//   save = 0                      : x0 | 2 layer slots used as a ring                                  (inference)
//   save = 1, grad_checkpoint = 0 : x0 | L layer slots -- everything backward needs is kept            (default)
//   save = 1, grad_checkpoint = 1 : x0 | L layer OUTPUTS [Tp,H] | 2 layer slots (ring) -- only every layer's input is kept
//                                   (torch.utils.checkpoint per BertLayer, SimANS/model/models.py:73-74); backward re-runs
//                                   a layer's forward into ring slot 0 (same stateless dropout masks) before its backward
// followed by the [CLS]-only last layer's compact tensors.
struct Act {
  char* base;
  size_t Tp;
  bool ckpt, ring;              // ring: two slots, layer l in slot l & 1
  XS x0;
  size_t kept, kept_stride;     // checkpoint mode: the layer outputs (offset of the first, stride)
  size_t slots, slot_stride;
  ClsExtra extra;
  size_t bytes;
};
static Act walk_act(const simx_bert_cfg* c, void* act, int T, int nseq, int save) {
  Act A = {};
  A.base = (char*)act;
  A.Tp = (size_t)rows_cap(T);
  A.ckpt = save && c->grad_checkpoint != 0;
  A.ring = !save || A.ckpt;
  Carver k{A.base, 0};
  A.x0 = walk_xs(c, k, A.Tp);
  if (A.ckpt) {
    A.kept = k.off;
    walk_xs(c, k, A.Tp);
    A.kept_stride = k.repeat(A.kept, (size_t)c->layers);
  }
  A.slots = k.off;
  walk_alayer(c, k, A.Tp);
  A.slot_stride = k.repeat(A.slots, A.ring ? 2 : (size_t)c->layers);
  A.extra = walk_cls_extra(c, k, nseq > 0 ? (size_t)nseq : A.Tp);
  A.bytes = k.off;
  return A;
}
extern "C" size_t simx_bert_act_bytes(const simx_bert_cfg* c, int T, int nseq, int save_for_bwd) {
  return cfg_ok(c) && T > 0 ? walk_act(c, nullptr, T, nseq, save_for_bwd).bytes : 0;
}
static ALayer act_slot(const simx_bert_cfg* c, const Act& A, int i) {
  Carver k{A.base, A.slots + (size_t)i * A.slot_stride};
  return walk_alayer(c, k, A.Tp);
}
// the slot layer l's FORWARD writes (checkpoint mode: ring slot l & 1, its output redirected to the kept array)
static ALayer alayer(const simx_bert_cfg* c, const Act& A, int l) {
  ALayer a = act_slot(c, A, A.ring ? l & 1 : l);
  if (A.ckpt) {
    Carver k{A.base, A.kept + (size_t)l * A.kept_stride};
    const XS out = walk_xs(c, k, A.Tp);
    a.xout = out.hi;
    a.xoutl = out.lo;
    a.xoutp = out.planes;
  }
  return a;
}
// the slot layer l's BACKWARD reads (checkpoint mode: the layer is RE-COMPUTED into ring slot 0, its own xout)
static ALayer alayer_bwd(const simx_bert_cfg* c, const Act& A, int l) { return A.ckpt ? act_slot(c, A, 0) : alayer(c, A, l); }
// input of layer l (= output of layer l-1, or the embedding output)
static XS layer_input(const simx_bert_cfg* c, const Act& A, int l) {
  if (l == 0) return A.x0;
  const ALayer p = alayer(c, A, l - 1);
  return XS{p.xout, p.xoutl, p.xoutp};
}

static size_t tn_ws_max(const simx_bert_cfg* c, int T) {
  const int H = c->hidden, F = c->inter;
  size_t m = simx_gemm_tn_workspace_bytes(3 * H, H, T);
  size_t v = simx_gemm_tn_workspace_bytes(H, H, T); if (v > m) m = v;
  v = simx_gemm_tn_workspace_bytes(F, H, T); if (v > m) m = v;
  v = simx_gemm_tn_workspace_bytes(H, F, T); if (v > m) m = v;
  if (pl_weights(c)) {
    v = simx_gemm_tn_planes_workspace_bytes(3 * H, H, T); if (v > m) m = v;
    v = simx_gemm_tn_planes_workspace_bytes(F, H, T); if (v > m) m = v;
    v = simx_gemm_tn_planes_workspace_bytes(H, F, T); if (v > m) m = v;
  }
  return m;
}
// Backward scratch.  bufB carries the gradient w.r.t. the current layer's OUTPUT from one layer to the next -- and from one
// simx_bert_bwd_range call to the next (the caller keeps `scratch` alive and untouched between the parts); bufA is the gradient
// of the residual branch; bufC the dropout-masked copy of dz (only with hidden dropout; always, as bf16 planes, in a plane tower)
struct Scratch { char *bufA, *bufB, *bufC, *du, *dqkv, *tnws, *e0, *e1, *e2, *xconv; size_t tnws_bytes, bytes; };
static Scratch walk_scratch(const simx_bert_cfg* c, void* scratch, int T, int nseq) {
  const size_t H = c->hidden, F = c->inter, e = esz(c->dtype);
  const size_t Tp = (size_t)rows_cap(T), n = nseq > 0 ? (size_t)nseq : Tp;
  Carver k{(char*)scratch, 0};
  Scratch s;
  s.bufA = k.take(Tp * H * e);
  s.bufB = k.take(Tp * H * e);
  s.bufC = k.take(Tp * H * e);
  s.du = k.take(Tp * F * e);
  s.dqkv = k.take(Tp * 3 * H * e);
  s.tnws_bytes = al(tn_ws_max(c, T));           // split-K slabs of the wgrad GEMMs
  s.tnws = k.take(s.tnws_bytes);
  s.e0 = k.take(n * H * e);                     // three [nseq,H] temporaries of the [CLS]-only last layer
  s.e1 = k.take(n * H * e);
  s.e2 = k.take(n * H * e);
  // operand planes: the bf16 plane pair of the activation a wgrad GEMM contracts against, converted per use
  s.xconv = pl_layout(c, Tp) ? k.take(Tp * F * 4) : nullptr;
  s.bytes = k.off;
  return s;
}
extern "C" size_t simx_bert_bwd_scratch_bytes(const simx_bert_cfg* c, int T, int nseq) {
  return cfg_ok(c) && T > 0 ? walk_scratch(c, nullptr, T, nseq).bytes : 0;
}

// ------------------------------------------------------------------------------------------ driver
#define RUN(call)            \
  do {                       \
    int rc__ = (call);       \
    if (rc__) return rc__;   \
  } while (0)

extern "C" int simx_bert_cast_weights(simx_stream_t stream, const simx_bert_cfg* c, const float* params, void* wcache) {
  SIMX_REQUIRE(cfg_ok(c), SIMX_ERR_BAD_SHAPE, "bert_cast_weights: bad config");
  SIMX_REQUIRE(params && wcache, SIMX_ERR_BAD_SHAPE, "bert_cast_weights: NULL buffer");
  const int H = c->hidden, F = c->inter;
  const bool f32 = c->dtype == SIMX_F32;
  if (pl_weights(c)) {                            // f32 transposes + both plane pairs of every dense weight, grouped launches
    static thread_local SimxSplitGroup sg;
    sg.n = 0;
    auto addp = [&](const float* w, int rows, int cols, const char* wT, const char* ph, const char* ptb) -> int {
      if (sg.n == SIMX_SPLIT_GROUP_MAX) { RUN(simx_split_weight_group((hipStream_t)stream, &sg)); sg.n = 0; }
      sg.job[sg.n++] = SimxSplitJob{w, (void*)ph, (void*)ptb, (float*)wT, rows, cols, 0, 0};
      return SIMX_OK;
    };
    for (int l = 0; l < c->layers; ++l) {
      const WLayer w = wlayer(c, params, wcache, l);
      RUN(addp(params + simx_bert_param_offset(c, l, SIMX_P_WQKV), 3 * H, H, w.wqkvT, w.wqkvP, w.wqkvTP));
      RUN(addp(params + simx_bert_param_offset(c, l, SIMX_P_WO), H, H, w.woT, w.woP, w.woTP));
      RUN(addp(params + simx_bert_param_offset(c, l, SIMX_P_W1), F, H, w.w1T, w.w1P, w.w1TP));
      RUN(addp(params + simx_bert_param_offset(c, l, SIMX_P_W2), H, F, w.w2T, w.w2P, w.w2TP));
    }
    if (sg.n) RUN(simx_split_weight_group((hipStream_t)stream, &sg));
    return SIMX_OK;
  }
  static thread_local SimxCastGroup g;              // (built in place, passed by value at the launch)
  g.n = 0;
  auto add = [&](const float* w, int rows, int cols, const char* out, const char* outT) -> int {
    if (g.n == SIMX_CAST_GROUP_MAX) { RUN(simx_transpose_cast_group((hipStream_t)stream, c->dtype, &g)); g.n = 0; }
    g.job[g.n++] = SimxCastJob{w, f32 ? nullptr : (void*)out, (void*)outT, rows, cols, 0, 0};
    return SIMX_OK;
  };
  for (int l = 0; l < c->layers; ++l) {
    const WLayer w = wlayer(c, params, wcache, l);
    RUN(add(params + simx_bert_param_offset(c, l, SIMX_P_WQKV), 3 * H, H, w.wqkv, w.wqkvT));
    RUN(add(params + simx_bert_param_offset(c, l, SIMX_P_WO), H, H, w.wo, w.woT));
    RUN(add(params + simx_bert_param_offset(c, l, SIMX_P_W1), F, H, w.w1, w.w1T));
    RUN(add(params + simx_bert_param_offset(c, l, SIMX_P_W2), H, F, w.w2, w.w2T));
  }
  if (g.n) RUN(simx_transpose_cast_group((hipStream_t)stream, c->dtype, &g));
  return SIMX_OK;
}

// dropout descriptor of (layer, site); layer -1 = embeddings
static simx_dropout drop_of(const simx_bert_cfg* c, int layer, int site) {
  simx_dropout d;
  d.p = site == 3 ? c->attn_dropout : c->hidden_dropout;
  d.seed = c->dropout_seed;
  d.stream = (uint32_t)((layer + 1) * 8 + site);
  return d;
}

static int check_io(const simx_bert_cfg* c, int nseq, int T, int max_len, const char* who) {
  SIMX_REQUIRE(cfg_ok(c), SIMX_ERR_BAD_SHAPE, "%s: bad config", who);
  SIMX_REQUIRE(c->hidden_dropout >= 0.f && c->hidden_dropout < 1.f && c->attn_dropout >= 0.f && c->attn_dropout < 1.f,
               SIMX_ERR_BAD_SHAPE, "%s: dropout probabilities must be in [0,1)", who);
  SIMX_REQUIRE(nseq > 0 && T >= nseq && max_len > 0 && max_len <= c->max_pos, SIMX_ERR_BAD_SHAPE,
               "%s: bad batch (nseq=%d T=%d max_len=%d max_pos=%d)", who, nseq, T, max_len, c->max_pos);
  return SIMX_OK;
}

// Head-major q/k/v (include/simx.h "head-major q / k / v"): chosen per tower when every kernel that touches the tensor has the
// form -- a 16-bit dtype, head size 64, sequences that the LDS-resident attention backward takes (<= 256), and a tower large
// enough for the persistent GEMMs (simx_gemm_hm_ok).  cfg->qkv_layout = 1 pins the token-major form (A/B measurements, tests);
// the choice is a function of (cfg, T, max_len) only, so a forward and its backward -- which receive the same per-call
// config copy -- always agree.
static int hm_rows_for(const simx_bert_cfg* c, int T, int Tp, int max_len) {
  if (c->qkv_layout == 1) return 0;
  const int d = c->hidden / c->heads;
  if (!simx_is16(c->dtype) || d != 64 || max_len > 256) return 0;
  return simx_gemm_hm_ok(Tp, c->hidden, T) ? Tp : 0;
}

// Hidden dropout is live <=> the LayerNorm backward writes the dropout-masked copy of dz (ln_bwd_kernel stores it under the
// REALISED threshold: make_drop runs 0 < p < 1/512 as no dropout).  The one predicate behind both the kernel's dz_masked
// argument and the buffer the dgrad / wgrad GEMMs read.
static bool hidden_drop_live(const simx_bert_cfg* c) {
  const simx_dropout d = drop_of(c, 0, 1);
  return make_drop(&d).thr != 0;
}

// What one forward / backward call hands to every layer
struct Ctx {
  hipStream_t stream;
  const simx_bert_cfg* c;
  const float* params;
  float* grads;
  const void* wcache;
  const int32_t* cu;
  int nseq, T, Tp, max_len;
  int hm;               // rows of the head-major q / k / v tensor (hm_rows_for), 0 = token-major
  const float* gs;      // fp16 engine: activation gradients travel multiplied by the loss scale S (gs = {S, 1/S} on the device); the
                        // kernels that accumulate into `grads` multiply by 1/S, so `grads` holds true gradients (simx.h "gradient scale")
  int gdt;              // fp32 engine: the dense GEMMs run on the 16-bit matrix cores from fp16 hi + lo splits of their f32 operands unless
                        // the config asks for exact f32 products (simx.h SIMX_F32_SPLIT_H; every other kernel of the layer is plain f32)
  int gdb;              // ... and the dgrad / wgrad GEMMs from bf16 splits (gradients need f32's exponent range; simx.h SIMX_F32_SPLIT_B)
  Act A;
  const float* p(int l, int w) const { return params + simx_bert_param_offset(c, l, w); }
  float* g(int l, int w) const { return grads + simx_bert_param_offset(c, l, w); }
};
static Ctx make_ctx(simx_stream_t stream, const simx_bert_cfg* c, const float* params, float* grads, const void* wcache, const int32_t* cu,
                    int nseq, int T, int max_len, void* act, int save) {
  Ctx cx;
  cx.stream = (hipStream_t)stream; cx.c = c; cx.params = params; cx.grads = grads; cx.wcache = wcache; cx.cu = cu;
  cx.nseq = nseq; cx.T = T; cx.Tp = rows_cap(T); cx.max_len = max_len;
  cx.hm = hm_rows_for(c, T, cx.Tp, max_len);
  cx.gs = c->dtype == SIMX_F16 ? c->grad_scale : nullptr;
  const bool split = c->dtype == SIMX_F32 && c->f32_gemm == 0;
  cx.gdt = split ? SIMX_F32_SPLIT_H : c->dtype;
  cx.gdb = split ? SIMX_F32_SPLIT_B : c->dtype;
  cx.A = walk_act(c, act, T, nseq, save);
  return cx;
}

// ---- forward: one encoder layer, x [Tp,H] -> a.xout (a = the slot it writes), in one of three forms.  `keep`: backward will read
// this slot (the pre-activation u is stored).

// Last layer, [CLS] rows only: row s of every [nseq, .] buffer below is the sequence's token 0 (row cu[s] of the
// full tensors).  Only K and V are projected for every token; Q, the attention core and everything after it run
// for the one query per sequence that is read.  Same arithmetic as the full path -- dropout masks stay keyed by
// the ORIGINAL row index.  z1, x1, u, h, z2, xout of this layer hold [nseq, .] tensors in their usual slots; q and the
// attention context of the [CLS] rows go to the compact tensors behind the slots.
static int layer_fwd_cls(const Ctx& cx, int l, const XS& x, const ALayer& a, float* cls_out) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, F = c->inter, dt = c->dtype, d = H / c->heads, nseq = cx.nseq, gdt = cx.gdt;
  const size_t e = esz(dt);
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const simx_dropout d1 = drop_of(c, l, 1), d2 = drop_of(c, l, 2), d3 = drop_of(c, l, 3);
  const ClsExtra& ex = cx.A.extra;
  if (cx.hm)      // K, V planes [heads, 3*heads) of the head-major tensor
    RUN(simx_gemm_nt_hm(cx.stream, dt, cx.Tp, 2 * H, H, x.hi, H, w.wqkv + (size_t)H * H * e, H, a.qkv + (size_t)c->heads * cx.hm * 64 * e, 64,
                        cx.p(l, SIMX_P_BQKV) + H, nullptr, 0, nullptr, 0, cx.hm));
  else
    RUN(simx_gemm_nt(cx.stream, gdt, cx.Tp, 2 * H, H, x.hi, H, w.wqkv + (size_t)H * H * e, H, a.qkv + (size_t)H * e, 3 * H,
                     cx.p(l, SIMX_P_BQKV) + H, nullptr, 0, SIMX_EPI_NONE, nullptr, 0, nullptr, 0));
  RUN(simx_rows_copy(cx.stream, dt, dt, nseq, H, cx.cu, nullptr, x.hi, ex.ytmp));
  RUN(simx_gemm_nt(cx.stream, gdt, nseq, H, H, ex.ytmp, H, w.wqkv, H, ex.qc, H, cx.p(l, SIMX_P_BQKV), nullptr, 0, SIMX_EPI_NONE, nullptr, 0,
                   nullptr, 0));
  RUN(simx_mha_cls_fwd_hm(cx.stream, dt, nseq, c->heads, d, cx.cu, cx.max_len, cx.T, ex.qc, a.qkv, ex.ctxc, &d3, cx.hm));
  RUN(simx_gemm_nt(cx.stream, gdt, nseq, H, H, ex.ctxc, H, w.wo, H, ex.ytmp, H, cx.p(l, SIMX_P_BO), nullptr, 0, SIMX_EPI_NONE, nullptr, 0,
                   nullptr, 0));
  // stream_lo: the [CLS] rows of the layer input (16-bit values + correction bytes) are gathered into xg / xgl, the dense outputs
  // are dropped WITHOUT their residual, the LayerNorm kernels add the residual in f32, and the embeddings leave as
  // f32(hi + correction) -- never rounded to 16 bits.  Otherwise the residual rides in simx_drop_residual_rows.
  const bool sl = stream_lo(c);
  if (sl) RUN(simx_stream_rows(cx.stream, dt, nseq, H, cx.cu, x.hi, x.lo, ex.xg, ex.xgl, nullptr));
  RUN(simx_drop_residual_rows(cx.stream, dt, nseq, H, ex.ytmp, sl ? nullptr : x.hi, sl ? nullptr : cx.cu, cx.cu, &d1, a.z1));
  RUN(simx_ln_fwd_res(cx.stream, dt, nseq, H, a.z1, sl ? ex.xg : nullptr, sl ? ex.xgl : nullptr, cx.p(l, SIMX_P_LN1_G), cx.p(l, SIMX_P_LN1_B), c->eps,
                      a.x1, a.x1l));
  RUN(simx_gemm_nt(cx.stream, gdt, nseq, F, H, a.x1, H, w.w1, H, a.u, F, cx.p(l, SIMX_P_B1), nullptr, 0, SIMX_EPI_GELU, nullptr, 0, a.h, F));
  RUN(simx_gemm_nt(cx.stream, gdt, nseq, H, F, a.h, F, w.w2, F, ex.ytmp, H, cx.p(l, SIMX_P_B2), nullptr, 0, SIMX_EPI_NONE, nullptr, 0,
                   nullptr, 0));
  RUN(simx_drop_residual_rows(cx.stream, dt, nseq, H, ex.ytmp, sl ? nullptr : a.x1, nullptr, cx.cu, &d2, a.z2));
  RUN(simx_ln_fwd_res(cx.stream, dt, nseq, H, a.z2, sl ? a.x1 : nullptr, sl ? a.x1l : nullptr, cx.p(l, SIMX_P_LN2_G), cx.p(l, SIMX_P_LN2_B), c->eps,
                      a.xout, a.xoutl));
  if (!cls_out) return SIMX_OK;
  if (sl) return simx_stream_rows(cx.stream, dt, nseq, H, nullptr, a.xout, a.xoutl, nullptr, nullptr, cls_out);
  return simx_rows_copy(cx.stream, dt, SIMX_F32, nseq, H, nullptr, nullptr, a.xout, cls_out);
}

// fp32 engine on operand planes: every GEMM operand is a 16-bit plane pair written by its producer -- x.planes by the previous
// LayerNorm, ctx by the attention kernel, x1p by LayerNorm, h by the FFN-in epilogue; f32 forms exist where an
// elementwise consumer needs them (residuals x / x1, q/k/v, the pre-LayerNorm sums, gelu')
static int layer_fwd_planes(const Ctx& cx, int l, const XS& x, const ALayer& a, int keep) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, F = c->inter, d = H / c->heads, T = cx.T, Tp = cx.Tp;
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const simx_dropout d1 = drop_of(c, l, 1), d2 = drop_of(c, l, 2), d3 = drop_of(c, l, 3);
  const long psH = (long)Tp * H, psF = (long)Tp * F;
  if (simx_mha_x3_ok(d, cx.max_len)) {
    // q / k / v leave the projection as an fp16 plane pair (no f32 form) and the attention products run on the 16-bit
    // matrix cores from pairs (csrc/attention_x3.hip); longer sequences keep f32 q / k / v and the chunked f32 MFMA kernels
    RUN(simx_gemm_nt_planes(cx.stream, SIMX_F16, SIMX_EPI_NONE_PLANES, Tp, 3 * H, H, x.planes, H, psH, w.wqkvP, H, 3L * H * H, nullptr, 3 * H,
                            cx.p(l, SIMX_P_BQKV), nullptr, 0, a.qkv, 3 * H, (long)Tp * 3 * H, nullptr));
    RUN(simx_mha_fwd_x3(cx.stream, cx.nseq, c->heads, d, cx.cu, cx.max_len, T, a.qkv, (long)Tp * 3 * H, a.ctx, psH, a.lse, &d3));
  } else {
    RUN(simx_gemm_nt_planes(cx.stream, SIMX_F16, SIMX_EPI_NONE, Tp, 3 * H, H, x.planes, H, psH, w.wqkvP, H, 3L * H * H, (float*)a.qkv, 3 * H,
                            cx.p(l, SIMX_P_BQKV), nullptr, 0, nullptr, 0, 0, nullptr));
    RUN(simx_mha_fwd_planes(cx.stream, cx.nseq, c->heads, d, cx.cu, cx.max_len, T, (const float*)a.qkv, a.ctx, psH, a.lse, &d3));
  }
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_F16, SIMX_EPI_NONE, Tp, H, H, a.ctx, H, psH, w.woP, H, (long)H * H, (float*)a.z1, H, cx.p(l, SIMX_P_BO),
                          (const float*)x.hi, H, nullptr, 0, 0, &d1));
  RUN(simx_ln_fwd_planes(cx.stream, T, H, (const float*)a.z1, cx.p(l, SIMX_P_LN1_G), cx.p(l, SIMX_P_LN1_B), c->eps, (float*)a.x1, a.x1p, psH));
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_F16, keep ? SIMX_EPI_GELU : SIMX_EPI_GELU_INFER, Tp, F, H, a.x1p, H, psH, w.w1P, H, (long)F * H,
                          (float*)a.u, F, cx.p(l, SIMX_P_B1), nullptr, 0, a.h, F, psF, nullptr));
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_F16, SIMX_EPI_NONE, Tp, H, F, a.h, F, psF, w.w2P, F, (long)H * F, (float*)a.z2, H, cx.p(l, SIMX_P_B2),
                          (const float*)a.x1, H, nullptr, 0, 0, &d2));
  return simx_ln_fwd_planes(cx.stream, T, H, (const float*)a.z2, cx.p(l, SIMX_P_LN2_G), cx.p(l, SIMX_P_LN2_B), c->eps, (float*)a.xout, a.xoutp, psH);
}

// the 16-bit engines and the fp32 engine on register-split (or exact f32) GEMMs
static int layer_fwd_dense(const Ctx& cx, int l, const XS& x, const ALayer& a, int keep) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, F = c->inter, dt = c->dtype, d = H / c->heads, T = cx.T, Tp = cx.Tp, gdt = cx.gdt;
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const simx_dropout d1 = drop_of(c, l, 1), d2 = drop_of(c, l, 2), d3 = drop_of(c, l, 3);
  if (cx.hm)
    RUN(simx_gemm_nt_hm(cx.stream, dt, Tp, 3 * H, H, x.hi, H, w.wqkv, H, a.qkv, 64, cx.p(l, SIMX_P_BQKV), nullptr, 0, nullptr, 0, cx.hm));
  else
    RUN(simx_gemm_nt(cx.stream, gdt, Tp, 3 * H, H, x.hi, H, w.wqkv, H, a.qkv, 3 * H, cx.p(l, SIMX_P_BQKV), nullptr, 0, SIMX_EPI_NONE,
                     nullptr, 0, nullptr, 0));
  RUN(simx_mha_fwd_hm(cx.stream, dt, cx.nseq, c->heads, d, cx.cu, cx.max_len, T, a.qkv, a.ctx, a.lse, &d3, cx.hm));
  // stream_lo: the dense output leaves without the residual (a plain bias + dropout epilogue) and the LayerNorm kernel sums
  // dense + x_hi + x_lo in f32; otherwise the residual rides in the GEMM epilogue and z1 is the LayerNorm input itself
  const bool sl = stream_lo(c);
  RUN(simx_gemm_nt_ex(cx.stream, gdt, Tp, H, H, a.ctx, H, w.wo, H, a.z1, H, cx.p(l, SIMX_P_BO), sl ? nullptr : x.hi, H, SIMX_EPI_NONE, nullptr, 0,
                      nullptr, 0, &d1));
  RUN(simx_ln_fwd_res(cx.stream, dt, T, H, a.z1, sl ? x.hi : nullptr, sl ? x.lo : nullptr, cx.p(l, SIMX_P_LN1_G), cx.p(l, SIMX_P_LN1_B), c->eps, a.x1,
                      a.x1l));
  RUN(simx_gemm_nt(cx.stream, gdt, Tp, F, H, a.x1, H, w.w1, H, a.u, F, cx.p(l, SIMX_P_B1), nullptr, 0,
                   keep ? SIMX_EPI_GELU : SIMX_EPI_GELU_INFER, nullptr, 0, a.h, F));   // no backward from this slot: u has no reader
  RUN(simx_gemm_nt_ex(cx.stream, gdt, Tp, H, F, a.h, F, w.w2, F, a.z2, H, cx.p(l, SIMX_P_B2), sl ? nullptr : a.x1, H, SIMX_EPI_NONE, nullptr, 0,
                      nullptr, 0, &d2));
  return simx_ln_fwd_res(cx.stream, dt, T, H, a.z2, sl ? a.x1 : nullptr, sl ? a.x1l : nullptr, cx.p(l, SIMX_P_LN2_G), cx.p(l, SIMX_P_LN2_B), c->eps,
                         a.xout, a.xoutl);
}

static int layer_fwd(const Ctx& cx, int l, const XS& x, const ALayer& a, int keep, bool cls_form, float* cls_out) {
  if (cls_form) return layer_fwd_cls(cx, l, x, a, cls_out);
  if (pl_run(cx.c, cx.Tp, cx.max_len)) return layer_fwd_planes(cx, l, x, a, keep);
  return layer_fwd_dense(cx, l, x, a, keep);
}

// [CLS] taps (simx.h simx_bert_fwd_taps): strictly ascending layer indices in [0, layers), with the buffer they fill / are read from
static int check_taps(const simx_bert_cfg* c, const int32_t* tap_layers, int ntap, const float* tap_buf, const char* who) {
  SIMX_REQUIRE(ntap >= 0 && (ntap == 0 || (tap_layers && tap_buf)), SIMX_ERR_BAD_SHAPE, "%s: %d taps without their layers / buffer", who, ntap);
  for (int k = 0; k < ntap; ++k)
    SIMX_REQUIRE(tap_layers[k] >= 0 && tap_layers[k] < c->layers && (k == 0 || tap_layers[k] > tap_layers[k - 1]), SIMX_ERR_BAD_SHAPE,
                 "%s: tap_layers must be strictly ascending in [0, %d)", who, c->layers);
  return SIMX_OK;
}
// slot of the tap on layer l, -1 = none
static int tap_slot(const int32_t* tap_layers, int ntap, int l) {
  for (int k = 0; k < ntap; ++k)
    if (tap_layers[k] == l) return k;
  return -1;
}
// the [CLS] rows of a full residual-stream tensor as f32 (a stream_lo tower: hi + correction byte)
static int cls_rows_out(const Ctx& cx, const XS& x, float* out) {
  if (x.lo) return simx_stream_rows(cx.stream, cx.c->dtype, cx.nseq, cx.c->hidden, cx.cu, x.hi, x.lo, nullptr, nullptr, out);
  return simx_cls_gather(cx.stream, cx.c->dtype, cx.nseq, cx.c->hidden, cx.cu, x.hi, out);
}

static int bert_fwd(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache, const int32_t* ids,
                    const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len, void* act, size_t act_bytes, int save,
                    float* cls_out, void* hidden_out, const int32_t* tap_layers, int ntap, float* tap_cls) {
  RUN(check_io(c, nseq, T, max_len, "bert_fwd"));
  RUN(check_taps(c, tap_layers, ntap, tap_cls, "bert_fwd"));
  SIMX_REQUIRE(params && wcache && ids && pos_ids && cu && act, SIMX_ERR_BAD_SHAPE, "bert_fwd: NULL buffer");
  const Ctx cx = make_ctx(stream, c, params, nullptr, wcache, cu, nseq, T, max_len, act, save);
  SIMX_REQUIRE(act_bytes >= cx.A.bytes, SIMX_ERR_WORKSPACE, "bert_fwd: activation buffer %zu < %zu", act_bytes, cx.A.bytes);
  const int H = c->hidden, dt = c->dtype;
  XS x = cx.A.x0;
  {
    const simx_dropout d0 = drop_of(c, -1, 0);
    if (x.planes)
      RUN(simx_embed_ln_fwd_planes(stream, T, H, ids, pos_ids, cx.p(-1, SIMX_P_WORD), cx.p(-1, SIMX_P_POS), cx.p(-1, SIMX_P_TYPE),
                                   cx.p(-1, SIMX_P_EMB_LN_G), cx.p(-1, SIMX_P_EMB_LN_B), c->eps, (float*)x.hi, x.planes, (long)cx.Tp * H, &d0));
    else
      RUN(simx_embed_ln_fwd_lo(stream, dt, T, H, ids, pos_ids, cx.p(-1, SIMX_P_WORD), cx.p(-1, SIMX_P_POS), cx.p(-1, SIMX_P_TYPE),
                               cx.p(-1, SIMX_P_EMB_LN_G), cx.p(-1, SIMX_P_EMB_LN_B), c->eps, x.hi, x.lo, &d0));
  }
  const bool cls_only = c->cls_only_last_layer != 0;
  SIMX_REQUIRE(!(cls_only && hidden_out), SIMX_ERR_BAD_SHAPE, "bert_fwd: cls_only_last_layer leaves no full hidden state to return");
  // a tap on the last layer is the embedding itself: computed once (into cls_out when the caller wants both), then copied
  const int last_k = tap_slot(tap_layers, ntap, c->layers - 1);
  float* last_tap = last_k >= 0 ? tap_cls + (size_t)last_k * nseq * H : nullptr;
  float* emb_out = cls_out ? cls_out : last_tap;
  for (int l = 0; l < c->layers; ++l) {
    const ALayer a = alayer(c, cx.A, l);
    const bool cls_form = cls_only && l == c->layers - 1;
    // (checkpoint mode: the slot is recomputed by backward, so the forward runs it in its inference form)
    RUN(layer_fwd(cx, l, x, a, save && !cx.A.ckpt, cls_form, emb_out));
    if (cls_form) break;
    x = XS{a.xout, a.xoutl, a.xoutp};
    const int k = l < c->layers - 1 ? tap_slot(tap_layers, ntap, l) : -1;
    if (k >= 0) RUN(cls_rows_out(cx, x, tap_cls + (size_t)k * nseq * H));
  }
  // (a stream_lo tower: the embeddings are f32(hi + correction byte), as the [CLS]-only last layer returns them -- the same
  // precision whichever form the last layer ran in)
  if (emb_out && !cls_only) RUN(cls_rows_out(cx, x, emb_out));
  if (last_tap && last_tap != emb_out &&
      hipMemcpyAsync(last_tap, emb_out, (size_t)nseq * H * sizeof(float), hipMemcpyDeviceToDevice, cx.stream) != hipSuccess) {
    simx_set_error("bert_fwd: copy of the last layer's tap failed");
    return SIMX_ERR_HIP;
  }
  if (hidden_out) {
    if (hipMemcpyAsync(hidden_out, x.hi, (size_t)T * H * esz(dt), hipMemcpyDeviceToDevice, cx.stream) != hipSuccess) {
      simx_set_error("bert_fwd: copy of last hidden state failed");
      return SIMX_ERR_HIP;
    }
  }
  return SIMX_OK;
}

extern "C" int simx_bert_fwd(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                             const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                             void* act, size_t act_bytes, int save, float* cls_out, void* hidden_out) {
  return bert_fwd(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, act, act_bytes, save, cls_out, hidden_out, nullptr, 0, nullptr);
}
extern "C" int simx_bert_fwd_taps(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                                  const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                                  void* act, size_t act_bytes, int save, float* cls_out, void* hidden_out, const int32_t* tap_layers,
                                  int ntap, float* tap_cls) {
  return bert_fwd(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, act, act_bytes, save, cls_out, hidden_out, tap_layers, ntap,
                  tap_cls);
}

// ---- backward: the three layer forms, mirroring the forwards.  On entry s.bufB holds the gradient w.r.t. the layer's output, on
// exit the gradient w.r.t. its input (full [T,H] tensors, except on entry to the [CLS] form).

// The post-attention half of a layer's backward -- output LayerNorm, FFN, attention-output LayerNorm, Wo -- on `n` rows
// (`np`: the row count of the NT GEMMs).  ctx: the attention context the Wo wgrad contracts against; res: the layer's input
// rows (read with stream_lo only: the residual of the attention-output LayerNorm); keys: the rows' dropout keys (NULL: the row
// index); dctx: where the gradient of the attention context goes.  Leaves the gradient of the residual branch in s.bufA.
struct PostRows { int n, np; const char* ctx; const char *res, *resl; const int32_t* keys; char* dctx; };
static int layer_bwd_post(const Ctx& cx, const Scratch& s, int l, const WLayer& w, const ALayer& a, const PostRows& r) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, F = c->inter, dt = c->dtype, gdb = cx.gdb;
  const simx_dropout d1 = drop_of(c, l, 1), d2 = drop_of(c, l, 2);
  const bool sl = stream_lo(c);
  // gradient of the (dropped) dense output: the masked copy when hidden dropout is live, else dz itself
  char* dz_masked = hidden_drop_live(c) ? s.bufC : nullptr;
  const char* dzm = dz_masked ? dz_masked : s.bufA;
  // output LayerNorm : dz2, dgamma2, dbeta2, db2
  RUN(simx_ln_bwd_res(cx.stream, dt, r.n, H, a.z2, sl ? a.x1 : nullptr, sl ? a.x1l : nullptr, cx.p(l, SIMX_P_LN2_G), c->eps, s.bufB, s.bufA,
                      dz_masked, cx.g(l, SIMX_P_LN2_G), cx.g(l, SIMX_P_LN2_B), cx.g(l, SIMX_P_B2), &d2, r.keys, cx.gs));
  // du = (dz2m . W2) * gelu'(u)
  RUN(simx_gemm_nt(cx.stream, gdb, r.np, F, H, dzm, H, w.w2T, H, s.du, F, nullptr, nullptr, 0, SIMX_EPI_DGELU, a.u, F, nullptr, 0));
  RUN(simx_gemm_tn_gs(cx.stream, gdb, H, F, r.n, dzm, H, a.h, F, cx.g(l, SIMX_P_W2), F, 1, s.tnws, s.tnws_bytes, nullptr, 0, cx.gs));
  // dx1 = du . W1 + dz2
  RUN(simx_gemm_nt(cx.stream, gdb, r.np, H, F, s.du, F, w.w1T, F, s.bufB, H, nullptr, s.bufA, H, SIMX_EPI_NONE, nullptr, 0, nullptr, 0));
  RUN(simx_gemm_tn_gs(cx.stream, gdb, F, H, r.n, s.du, F, a.x1, H, cx.g(l, SIMX_P_W1), H, 1, s.tnws, s.tnws_bytes, cx.g(l, SIMX_P_B1), 0, cx.gs));
  // attention-output LayerNorm : dz1, dgamma1, dbeta1, dbo
  RUN(simx_ln_bwd_res(cx.stream, dt, r.n, H, a.z1, sl ? r.res : nullptr, sl ? r.resl : nullptr, cx.p(l, SIMX_P_LN1_G), c->eps, s.bufB, s.bufA,
                      dz_masked, cx.g(l, SIMX_P_LN1_G), cx.g(l, SIMX_P_LN1_B), cx.g(l, SIMX_P_BO), &d1, r.keys, cx.gs));
  // dctx = dz1m . Wo
  RUN(simx_gemm_nt(cx.stream, gdb, r.np, H, H, dzm, H, w.woT, H, r.dctx, H, nullptr, nullptr, 0, SIMX_EPI_NONE, nullptr, 0, nullptr, 0));
  return simx_gemm_tn_gs(cx.stream, gdb, H, H, r.n, dzm, H, r.ctx, H, cx.g(l, SIMX_P_WO), H, 1, s.tnws, s.tnws_bytes, nullptr, 0, cx.gs);
}

// mirror of the forward's [CLS]-only last layer: everything up to the attention core runs on nseq rows
static int layer_bwd_cls(const Ctx& cx, const Scratch& s, int l, const float* dcls) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, dt = c->dtype, d = H / c->heads, nseq = cx.nseq, T = cx.T, Tp = cx.Tp, hm = cx.hm, gdb = cx.gdb;
  const size_t e = esz(dt);
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const XS x = layer_input(c, cx.A, l);
  const ALayer a = alayer_bwd(c, cx.A, l);
  if (cx.A.ckpt) RUN(layer_fwd(cx, l, x, a, 1, true, nullptr));
  const simx_dropout d3 = drop_of(c, l, 3);
  const ClsExtra& ex = cx.A.extra;                    // qc, ctxc and (stream_lo) xg / xgl: saved by the forward
  RUN(simx_rows_copy_gs(cx.stream, SIMX_F32, dt, nseq, H, nullptr, nullptr, dcls, s.bufB, cx.gs));
  // e1 = dctx (gradient of the attention context, [CLS] rows), bufA[0:nseq] = gradient of the residual branch
  RUN(layer_bwd_post(cx, s, l, w, a, PostRows{nseq, nseq, ex.ctxc, ex.xg, ex.xgl, cx.cu, s.e1}));
  // attention core for the one query per sequence: e0 = dq [nseq,H]; dK, dV for every token -> dqkv[:, H:3H]
  RUN(simx_mha_cls_bwd_hm(cx.stream, dt, nseq, c->heads, d, cx.cu, cx.max_len, T, ex.qc, a.qkv, s.e1, s.e0, s.dqkv, &d3, hm));
  // Q projection ([CLS] rows): dWq, dbq, and dx = dq . Wq + (residual-branch gradient), still compact
  RUN(simx_rows_copy(cx.stream, dt, dt, nseq, H, cx.cu, nullptr, x.hi, s.e2));
  RUN(simx_gemm_tn_gs(cx.stream, gdb, H, H, nseq, s.e0, H, s.e2, H, cx.g(l, SIMX_P_WQKV), H, 1, s.tnws, s.tnws_bytes, cx.g(l, SIMX_P_BQKV), 0, cx.gs));
  RUN(simx_gemm_nt(cx.stream, gdb, nseq, H, H, s.e0, H, w.wqkvT, 3 * H, s.e1, H, nullptr, s.bufA, H, SIMX_EPI_NONE, nullptr, 0, nullptr, 0));
  // back to full tensors: that gradient is zero outside the [CLS] rows
  if (hipMemsetAsync(s.bufA, 0, (size_t)T * H * e, cx.stream) != hipSuccess) {
    simx_set_error("bert_bwd: memset failed");
    return SIMX_ERR_HIP;
  }
  RUN(simx_rows_copy(cx.stream, dt, dt, nseq, H, nullptr, cx.cu, s.e1, s.bufA));
  // K, V projections (every token): dx += dkv . Wkv ; dWkv, dbkv
  if (hm) {
    const char* dkv = s.dqkv + (size_t)c->heads * hm * 64 * e;                  // planes [heads, 3*heads)
    RUN(simx_gemm_nt_hm(cx.stream, dt, Tp, H, 2 * H, dkv, 64, w.wqkvT + (size_t)H * e, 3 * H, s.bufB, H, nullptr, s.bufA, H, nullptr, hm, 0));
    return simx_gemm_tn_gs(cx.stream, gdb, 2 * H, H, T, dkv, 0, x.hi, H, cx.g(l, SIMX_P_WQKV) + (size_t)H * H, H, 1, s.tnws, s.tnws_bytes,
                           cx.g(l, SIMX_P_BQKV) + H, hm, cx.gs);
  }
  RUN(simx_gemm_nt(cx.stream, gdb, Tp, H, 2 * H, s.dqkv + (size_t)H * e, 3 * H, w.wqkvT + (size_t)H * e, 3 * H, s.bufB, H, nullptr, s.bufA, H,
                   SIMX_EPI_NONE, nullptr, 0, nullptr, 0));
  return simx_gemm_tn_gs(cx.stream, gdb, 2 * H, H, T, s.dqkv + (size_t)H * e, 3 * H, x.hi, H, cx.g(l, SIMX_P_WQKV) + (size_t)H * H, H, 1, s.tnws,
                         s.tnws_bytes, cx.g(l, SIMX_P_BQKV) + H, 0, cx.gs);
}

// fp32 engine on operand planes (see layer_fwd_planes): gradients that feed a GEMM leave their producer as bf16 plane pairs --
// bufC = dz (x dropout mask) from the LayerNorm backward, du from the DGELU epilogue, dqkv from the attention backward;
// the activation operand of each wgrad GEMM is converted to a bf16 pair into xconv right before its use
static int layer_bwd_planes(const Ctx& cx, const Scratch& s, int l) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, F = c->inter, d = H / c->heads, nseq = cx.nseq, T = cx.T, Tp = cx.Tp;
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const XS x = layer_input(c, cx.A, l);
  const ALayer a = alayer_bwd(c, cx.A, l);
  if (cx.A.ckpt) RUN(layer_fwd(cx, l, x, a, 1, false, nullptr));
  const simx_dropout d1 = drop_of(c, l, 1), d2 = drop_of(c, l, 2), d3 = drop_of(c, l, 3);
  const long psH = (long)Tp * H, psF = (long)Tp * F, ps3 = (long)Tp * 3 * H;
  RUN(simx_ln_bwd_planes(cx.stream, T, H, (const float*)a.z2, cx.p(l, SIMX_P_LN2_G), c->eps, (const float*)s.bufB, (float*)s.bufA, s.bufC, psH,
                         cx.g(l, SIMX_P_LN2_G), cx.g(l, SIMX_P_LN2_B), cx.g(l, SIMX_P_B2), &d2));
  // (the bias gradient of B1 = column sums of du comes out of this epilogue, so the W1 wgrad runs on the four-plane-stage
  // kernel, which carries no fused bias pass; the deterministic mode keeps the wgrad kernel's ordered pass)
  const bool b1_here = !simx_det();
  RUN(simx_gemm_nt_planes_cs(cx.stream, SIMX_BF16, SIMX_EPI_DGELU, Tp, F, H, s.bufC, H, psH, w.w2TP, H, (long)F * H, nullptr, F, nullptr,
                             (const float*)a.u, F, s.du, F, psF, nullptr, b1_here ? cx.g(l, SIMX_P_B1) : nullptr, T));
  RUN(simx_planes_from(cx.stream, SIMX_F16, SIMX_BF16, T, F, a.h, F, psF, s.xconv, F, psF));
  RUN(simx_gemm_tn_planes(cx.stream, H, F, T, s.bufC, H, psH, s.xconv, F, psF, cx.g(l, SIMX_P_W2), F, 1, s.tnws, s.tnws_bytes, nullptr));
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_BF16, SIMX_EPI_NONE, Tp, H, F, s.du, F, psF, w.w1TP, F, (long)H * F, (float*)s.bufB, H, nullptr,
                          (const float*)s.bufA, H, nullptr, 0, 0, nullptr));
  RUN(simx_planes_from(cx.stream, SIMX_F32, SIMX_BF16, T, H, a.x1, H, 0, s.xconv, H, psH));
  RUN(simx_gemm_tn_planes(cx.stream, F, H, T, s.du, F, psF, s.xconv, H, psH, cx.g(l, SIMX_P_W1), H, 1, s.tnws, s.tnws_bytes,
                          b1_here ? nullptr : cx.g(l, SIMX_P_B1)));
  RUN(simx_ln_bwd_planes(cx.stream, T, H, (const float*)a.z1, cx.p(l, SIMX_P_LN1_G), c->eps, (const float*)s.bufB, (float*)s.bufA, s.bufC, psH,
                         cx.g(l, SIMX_P_LN1_G), cx.g(l, SIMX_P_LN1_B), cx.g(l, SIMX_P_BO), &d1));
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_BF16, SIMX_EPI_NONE, Tp, H, H, s.bufC, H, psH, w.woTP, H, (long)H * H, (float*)s.bufB, H, nullptr, nullptr, 0,
                          nullptr, 0, 0, nullptr));
  RUN(simx_planes_from(cx.stream, SIMX_F16, SIMX_BF16, T, H, a.ctx, H, psH, s.xconv, H, psH));
  RUN(simx_gemm_tn_planes(cx.stream, H, H, T, s.bufC, H, psH, s.xconv, H, psH, cx.g(l, SIMX_P_WO), H, 1, s.tnws, s.tnws_bytes, nullptr));
  // (x3 attention: the QKV bias gradient = column sums of dq | dk | dv comes out of the attention backward, so the Wqkv wgrad
  // runs on the four-plane-stage kernel too; the deterministic mode keeps the wgrad kernel's ordered pass)
  const bool bqkv_here = simx_mha_x3_ok(d, cx.max_len) && !simx_det();
  if (simx_mha_x3_ok(d, cx.max_len))
    RUN(simx_mha_bwd_x3_bias(cx.stream, nseq, c->heads, d, cx.cu, cx.max_len, T, a.qkv, ps3, a.ctx, psH, a.lse, (const float*)s.bufB, s.dqkv, ps3, &d3,
                             bqkv_here ? cx.g(l, SIMX_P_BQKV) : nullptr));
  else
    RUN(simx_mha_bwd_planes(cx.stream, nseq, c->heads, d, cx.cu, cx.max_len, T, (const float*)a.qkv, a.ctx, psH, a.lse, (const float*)s.bufB, s.dqkv, ps3,
                            &d3));
  RUN(simx_gemm_nt_planes(cx.stream, SIMX_BF16, SIMX_EPI_NONE, Tp, H, 3 * H, s.dqkv, 3 * H, ps3, w.wqkvTP, 3 * H, 3L * H * H, (float*)s.bufB, H, nullptr,
                          (const float*)s.bufA, H, nullptr, 0, 0, nullptr));
  RUN(simx_planes_from(cx.stream, SIMX_F32, SIMX_BF16, T, H, x.hi, H, 0, s.xconv, H, psH));
  return simx_gemm_tn_planes(cx.stream, 3 * H, H, T, s.dqkv, 3 * H, ps3, s.xconv, H, psH, cx.g(l, SIMX_P_WQKV), H, 1, s.tnws, s.tnws_bytes,
                             bqkv_here ? nullptr : cx.g(l, SIMX_P_BQKV));
}

static int layer_bwd_dense(const Ctx& cx, const Scratch& s, int l) {
  const simx_bert_cfg* c = cx.c;
  const int H = c->hidden, dt = c->dtype, d = H / c->heads, T = cx.T, Tp = cx.Tp, hm = cx.hm, gdb = cx.gdb;
  const WLayer w = wlayer(c, cx.params, cx.wcache, l);
  const XS x = layer_input(c, cx.A, l);
  const ALayer a = alayer_bwd(c, cx.A, l);
  if (cx.A.ckpt) RUN(layer_fwd(cx, l, x, a, 1, false, nullptr));
  const simx_dropout d3 = drop_of(c, l, 3);
  RUN(layer_bwd_post(cx, s, l, w, a, PostRows{T, Tp, a.ctx, x.hi, x.lo, nullptr, s.bufB}));
  RUN(simx_mha_bwd_hm(cx.stream, dt, cx.nseq, c->heads, d, cx.cu, cx.max_len, T, a.qkv, a.ctx, a.lse, s.bufB, s.dqkv, &d3, hm));
  // dx = dqkv . Wqkv + dz1
  if (hm) {
    RUN(simx_gemm_nt_hm(cx.stream, dt, Tp, H, 3 * H, s.dqkv, 64, w.wqkvT, 3 * H, s.bufB, H, nullptr, s.bufA, H, nullptr, hm, 0));
    return simx_gemm_tn_gs(cx.stream, gdb, 3 * H, H, T, s.dqkv, 0, x.hi, H, cx.g(l, SIMX_P_WQKV), H, 1, s.tnws, s.tnws_bytes, cx.g(l, SIMX_P_BQKV), hm,
                           cx.gs);
  }
  RUN(simx_gemm_nt(cx.stream, gdb, Tp, H, 3 * H, s.dqkv, 3 * H, w.wqkvT, 3 * H, s.bufB, H, nullptr, s.bufA, H, SIMX_EPI_NONE, nullptr, 0,
                   nullptr, 0));
  return simx_gemm_tn_gs(cx.stream, gdb, 3 * H, H, T, s.dqkv, 3 * H, x.hi, H, cx.g(l, SIMX_P_WQKV), H, 1, s.tnws, s.tnws_bytes,
                         cx.g(l, SIMX_P_BQKV), 0, cx.gs);
}

extern "C" int simx_bert_bwd(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                             const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                             const void* act, size_t act_bytes, const float* dcls, float* grads, void* scratch,
                             size_t scratch_bytes) {
  return simx_bert_bwd_ex(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, act, act_bytes, dcls, nullptr, grads, scratch,
                          scratch_bytes);
}

extern "C" int simx_bert_bwd_ex(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                                const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                                const void* act, size_t act_bytes, const float* dcls, const void* dhidden, float* grads,
                                void* scratch, size_t scratch_bytes) {
  return simx_bert_bwd_range(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, const_cast<void*>(act), act_bytes, dcls,
                             dhidden, grads, scratch, scratch_bytes, c ? c->layers - 1 : 0, 0);
}

static int bert_bwd_range(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache, const int32_t* ids,
                          const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len, void* act, size_t act_bytes,
                          const float* dcls, const void* dhidden, float* grads, void* scratch, size_t scratch_bytes, int layer_hi,
                          int layer_lo, const int32_t* tap_layers, int ntap, const float* dtap_cls) {
  RUN(check_io(c, nseq, T, max_len, "bert_bwd"));
  RUN(check_taps(c, tap_layers, ntap, dtap_cls, "bert_bwd"));
  SIMX_REQUIRE(params && wcache && ids && pos_ids && cu && act && grads && scratch, SIMX_ERR_BAD_SHAPE, "bert_bwd: NULL buffer");
  SIMX_REQUIRE(layer_hi < c->layers && layer_lo >= 0 && layer_lo <= layer_hi, SIMX_ERR_BAD_SHAPE, "bert_bwd: bad layer range %d..%d",
               layer_hi, layer_lo);
  const bool top = layer_hi == c->layers - 1;
  SIMX_REQUIRE(!top || ((dcls != nullptr) != (dhidden != nullptr)), SIMX_ERR_BAD_SHAPE, "bert_bwd: pass exactly one of dcls / dhidden");
  SIMX_REQUIRE(!(dhidden && c->cls_only_last_layer), SIMX_ERR_BAD_SHAPE,
               "bert_bwd: a gradient for the whole hidden state needs the full last layer (cls_only_last_layer = 0)");
  const Ctx cx = make_ctx(stream, c, params, grads, wcache, cu, nseq, T, max_len, act, 1);
  const Scratch s = walk_scratch(c, scratch, T, nseq);
  SIMX_REQUIRE(act_bytes >= cx.A.bytes, SIMX_ERR_WORKSPACE, "bert_bwd: activation buffer too small");
  SIMX_REQUIRE(scratch_bytes >= s.bytes, SIMX_ERR_WORKSPACE, "bert_bwd: scratch %zu < %zu", scratch_bytes, s.bytes);
  const int H = c->hidden, dt = c->dtype;
  const bool pl = pl_run(c, cx.Tp, max_len);

  // gradient of the tap on layer l (f32 [nseq,H]), NULL = none
  auto dtap = [&](int l) -> const float* {
    const int k = tap_slot(tap_layers, ntap, l);
    return k >= 0 ? dtap_cls + (size_t)k * nseq * H : nullptr;
  };
  // a tap on the last layer is a second reader of the embedding: its gradient joins dcls in f32 before either enters the stack
  // (the sum lives in dqkv, which no kernel writes before the attention backward of the first layer differentiated)
  const float* dlast = top ? dtap(c->layers - 1) : nullptr;
  if (dlast && dcls) {
    float* sum = reinterpret_cast<float*>(s.dqkv);
    if (hipMemcpyAsync(sum, dcls, (size_t)nseq * H * sizeof(float), hipMemcpyDeviceToDevice, cx.stream) != hipSuccess) {
      simx_set_error("bert_bwd: copy of the embedding gradient failed");
      return SIMX_ERR_HIP;
    }
    RUN(simx_cls_rows_add_gs(stream, SIMX_F32, nseq, H, nullptr, dlast, sum, nullptr));
    dcls = sum;
    dlast = nullptr;
  }
  // the gradient w.r.t. the last hidden state -> bufB (the [CLS]-only last layer takes dcls itself)
  int l_top = layer_hi;
  if (top && c->cls_only_last_layer) {
    RUN(layer_bwd_cls(cx, s, l_top--, dcls));
  } else if (top && dhidden) {
    if (hipMemcpyAsync(s.bufB, dhidden, (size_t)T * H * esz(dt), hipMemcpyDeviceToDevice, cx.stream) != hipSuccess) {
      simx_set_error("bert_bwd: copy of the hidden-state gradient failed");
      return SIMX_ERR_HIP;
    }
  } else if (top) {
    RUN(simx_cls_scatter_gs(stream, dt, nseq, H, T, cu, dcls, s.bufB, cx.gs));            // g_x = d(loss)/d(last hidden)
  }
  if (dlast) RUN(simx_cls_rows_add_gs(stream, dt, nseq, H, cu, dlast, s.bufB, cx.gs));      // (dhidden form: no dcls to join)
  for (int l = l_top; l >= layer_lo; --l) {
    // the [CLS] rows of layer l's output have one more reader: += gs * dtap, before the layer is differentiated
    const float* dt_l = l < c->layers - 1 ? dtap(l) : nullptr;
    if (dt_l) RUN(simx_cls_rows_add_gs(stream, dt, nseq, H, cu, dt_l, s.bufB, cx.gs));
    RUN(pl ? layer_bwd_planes(cx, s, l) : layer_bwd_dense(cx, s, l));
  }
  if (layer_lo > 0) return SIMX_OK;               // the next part continues from bufB
  const simx_dropout d0 = drop_of(c, -1, 0);
  return simx_embed_ln_bwd_seq_gs(stream, dt, nseq, max_len, T, H, cu, ids, pos_ids, cx.p(-1, SIMX_P_WORD), cx.p(-1, SIMX_P_POS),
                                  cx.p(-1, SIMX_P_TYPE), cx.p(-1, SIMX_P_EMB_LN_G), c->eps, s.bufB, cx.g(-1, SIMX_P_WORD),
                                  cx.g(-1, SIMX_P_POS), cx.g(-1, SIMX_P_TYPE), cx.g(-1, SIMX_P_EMB_LN_G), cx.g(-1, SIMX_P_EMB_LN_B), &d0, cx.gs);
}

extern "C" int simx_bert_bwd_range(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                                   const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                                   void* act, size_t act_bytes, const float* dcls, const void* dhidden, float* grads,
                                   void* scratch, size_t scratch_bytes, int layer_hi, int layer_lo) {
  return bert_bwd_range(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, act, act_bytes, dcls, dhidden, grads, scratch,
                        scratch_bytes, layer_hi, layer_lo, nullptr, 0, nullptr);
}
extern "C" int simx_bert_bwd_taps(simx_stream_t stream, const simx_bert_cfg* c, const float* params, const void* wcache,
                                  const int32_t* ids, const int32_t* pos_ids, const int32_t* cu, int nseq, int T, int max_len,
                                  void* act, size_t act_bytes, const float* dcls, const void* dhidden, float* grads,
                                  void* scratch, size_t scratch_bytes, int layer_hi, int layer_lo, const int32_t* tap_layers,
                                  int ntap, const float* dtap_cls) {
  return bert_bwd_range(stream, c, params, wcache, ids, pos_ids, cu, nseq, T, max_len, act, act_bytes, dcls, dhidden, grads, scratch,
                        scratch_bytes, layer_hi, layer_lo, tap_layers, ntap, dtap_cls);
}
