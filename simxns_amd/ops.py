"""torch-facing wrappers of the f32 similarity / loss / sampler / optimiser kernels.

Each wrapper validates tensors, hands raw device pointers and the current HIP stream to the
C ABI (include/simx.h) and, where a gradient exists, ties the kernel's closed-form backward
 into autograd.  No wrapper has an eager fallback.
"""
import ctypes as C
import math

import torch

from . import _lib as L


def _f32c(t):
    if not t.is_cuda:
        raise L.SimxError("simxns_amd ops run only on a HIP device (no CPU fallback)")
    return t.contiguous().to(torch.float32)


# ------------------------------------------------------------------------------------------ M1 + L1/L2/L3/L6
class _SimLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, c, teacher, lp):
        q, c = _f32c(q), _f32c(c)
        B, H = q.shape
        D = c.shape[0] // B
        assert c.shape[0] == B * D and c.shape[1] == H
        teacher = _f32c(teacher) if teacher is not None else None
        sim = torch.empty(B, D, dtype=torch.float32, device=q.device)
        losses = torch.empty(4, dtype=torch.float32, device=q.device)
        dq, dc = torch.empty_like(q), torch.empty_like(c)
        L.call("simx_sim_loss_fwd_bwd", L.stream_ptr(), B, D, H, L.ptr(q), L.ptr(c), L.ptr(teacher), C.byref(lp),
               L.ptr(sim), L.ptr(losses), L.ptr(dq), L.ptr(dc))
        ctx.save_for_backward(dq, dc)
        ctx.mark_non_differentiable(sim)
        return losses[0], losses.detach(), sim

    @staticmethod
    def backward(ctx, g, g_all, g_sim):
        dq, dc = ctx.saved_tensors
        return dq * g, dc * g, None, None


class _LogitLossFn(torch.autograd.Function):
    """Loss on ready-made logits [B,D] (teacher CE, L6)."""

    @staticmethod
    def forward(ctx, logits, teacher, lp):
        z = _f32c(logits).clone()
        B, D = z.shape
        teacher = _f32c(teacher) if teacher is not None else None
        losses = torch.empty(4, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        L.call("simx_sim_loss_fwd_bwd", L.stream_ptr(), B, D, 0, None, None, L.ptr(teacher), C.byref(lp), L.ptr(z),
               L.ptr(losses), None, L.ptr(dz))
        ctx.save_for_backward(dz)
        return losses[0], losses.detach()

    @staticmethod
    def backward(ctx, g, g_all):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None


def _lp(kind, scale=1.0, temperature=1.0, adv_lambda=0.0, ce_w=0.0, kd_w=0.0, grad_accum=1.0, dkd_alpha=0.0, dkd_beta=0.0):
    return L.LossParams(kind, float(scale), float(temperature), float(adv_lambda), float(ce_w), float(kd_w),
                        float(grad_accum), float(dkd_alpha), float(dkd_beta))


# KD_type (PROD --KD_type) -> loss kind of the block form / kd_type of the all-pairs form
CROSS_KD_KINDS = {"KD_softmax": L.LOSS_CEKD, "KD_logit": L.LOSS_CE_LOGIT, "DKD": L.LOSS_CE_DKD, "prob_loss": L.LOSS_CE_PROB}
BI_KD_TYPES = {"KD_softmax": L.KD_SOFTMAX, "KD_logit": L.KD_LOGIT, "DKD": L.KD_DKD, "Bi_logit": L.KD_BI_LOGIT}


def _kd_kind(table, kd_type, dkd_alpha, dkd_beta):
    """Validated (kind, alpha, beta) of a kd_type; raises before anything touches the device."""
    if kd_type not in table:
        raise ValueError("kd_type %r: this loss knows %s" % (kd_type, ", ".join(sorted(table))))
    if kd_type != "DKD":
        return table[kd_type], 0.0, 0.0
    if dkd_alpha is None or dkd_beta is None:
        raise ValueError("kd_type 'DKD' needs dkd_alpha and dkd_beta")
    return table[kd_type], float(dkd_alpha), float(dkd_beta)


def kl_distill_loss(q, ctx_vectors, teacher_logits, temperature_distill=1.0, scale_simmila=False, grad_accum=1):
    """co_training_marco_train.py:199-217 in one kernel.  -> (loss/grad_accum, distill_loss, student_simila)."""
    scale = 1.0 / math.sqrt(q.shape[1]) if scale_simmila else 1.0
    loss, allv, sim = _SimLossFn.apply(q, ctx_vectors, teacher_logits,
                                       _lp(L.LOSS_KL, scale, temperature_distill, grad_accum=grad_accum))
    return loss, allv[1], sim


def wiki_normal_adv_loss(q, ctx_vectors, reranker_logits, temperature_normal=1.0, adv_lambda=0.0, scale_simmila=False,
                         grad_accum=1):
    """co_training_wiki_train.py:199-228.  -> (loss/grad_accum, normal_loss, adv_loss, retriever_simila)."""
    scale = 1.0 / math.sqrt(q.shape[1]) if scale_simmila else 1.0
    loss, allv, sim = _SimLossFn.apply(q, ctx_vectors, reranker_logits,
                                       _lp(L.LOSS_WIKI, scale, temperature_normal, adv_lambda, grad_accum=grad_accum))
    return loss, allv[1], allv[2], sim


def cross_kd_loss(q, ctx_vectors, relevance_logits, temperature=4.0, ce_weight=0.1, kd_weight=0.9, kd_type="KD_softmax",
                  dkd_alpha=None, dkd_beta=None):
    """PROD CrossBERTKDLoss.calc: ce_weight * hard + kd_weight * soft, soft chosen by ``kd_type`` (KD_softmax, KD_logit,
    DKD with ``dkd_alpha`` / ``dkd_beta``, prob_loss).  -> (loss, correct_count, hard, soft)."""
    kind, alpha, beta = _kd_kind(CROSS_KD_KINDS, kd_type, dkd_alpha, dkd_beta)
    loss, allv, _ = _SimLossFn.apply(q, ctx_vectors, relevance_logits,
                                     _lp(kind, 1.0, temperature, 0.0, ce_weight, kd_weight, dkd_alpha=alpha, dkd_beta=beta))
    return loss, allv[3], allv[1], allv[2]


def block_scores(q, ctx_vectors):
    """einsum('bh,bdh->bd') of query b against ITS OWN 1+N passages (no grad): [B, 1+N] f32."""
    with torch.no_grad():
        _, _, sim = _SimLossFn.apply(q.detach(), ctx_vectors.detach(), None, _lp(L.LOSS_CE))
    return sim


def pair_ce_loss(q, ctx_vectors):
    """-log_softmax(einsum('bh,bdh->bd'))[:,0].mean() (BiBertEncoder triplet form, models.py:111-118)."""
    loss, allv, _ = _SimLossFn.apply(q, ctx_vectors, None, _lp(L.LOSS_CE))
    return loss, allv[3]


def teacher_ce_loss(relevance_logits, grad_accum=1):
    """co_training_marco_train.py:228-236: CrossEntropy(logits, target 0).  -> (loss/grad_accum, contr_loss)."""
    loss, allv = _LogitLossFn.apply(relevance_logits, None, _lp(L.LOSS_CE, grad_accum=grad_accum))
    return loss, allv[1]


# ------------------------------------------------------------------------------------------ M2
def _scores_ws(Q, Cn, H, q_n, c_n, device):
    """split-K workspace of M2's backward products (None when the shapes need none)."""
    n = int(L.load().simx_scores_workspace_bytes(Q, Cn, H, q_n, c_n))
    return (torch.empty(n, dtype=torch.uint8, device=device) if n else None), n


class _ScoresFn(torch.autograd.Function):
    """The all-pairs losses.  kd: None for the NLL form, else (kd_type, teacher q, teacher ctx, T, ce_w, kd_w, alpha, beta)
    with the teacher's (constant) embeddings."""

    @staticmethod
    def forward(ctx, q, c, pos_idx, loss_scale, q_lo, q_n, c_lo, c_n, kd):
        q, c = _f32c(q), _f32c(c)
        Q, H = q.shape
        Cn = c.shape[0]
        if kd is not None:
            kd_type, tq, tc, T, ce_w, kd_w, alpha, beta = kd
            tq, tc = _f32c(tq.detach()), _f32c(tc.detach())
            bi = kd_type == L.KD_BI_LOGIT
            if bi and (tq.shape != q.shape or tc.shape != c.shape):
                raise ValueError("Bi_logit compares embeddings: teacher shapes %s / %s differ from the student's %s / %s"
                                 % (tuple(tq.shape), tuple(tc.shape), tuple(q.shape), tuple(c.shape)))
        pos = torch.as_tensor(pos_idx, dtype=torch.int32, device=q.device).contiguous()
        scores = torch.empty(Q, Cn, dtype=torch.float32, device=q.device)
        losses = torch.empty(4, dtype=torch.float32, device=q.device)
        dq, dc = torch.zeros_like(q), torch.zeros_like(c)
        ws, wsb = _scores_ws(Q, Cn, H, q_n, c_n, q.device)
        scale_slots = (float(loss_scale or 1.0), q_lo, q_n, c_lo, c_n)
        outs = (L.ptr(losses), C.c_void_p(dq.data_ptr() + q_lo * H * 4), C.c_void_p(dc.data_ptr() + c_lo * H * 4),
                L.ptr(ws) if wsb else None, wsb)
        if kd is None:
            L.call("simx_scores_nll_fwd_bwd", L.stream_ptr(), Q, Cn, H, L.ptr(q), L.ptr(c), L.ptr(pos), *scale_slots,
                   L.ptr(scores), None, *outs)
        else:
            tscores = None if bi else torch.empty(Q, Cn, dtype=torch.float32, device=q.device)
            L.call("simx_scores_kd_type_fwd_bwd", L.stream_ptr(), kd_type, Q, Cn, H, tq.shape[1], L.ptr(q), L.ptr(c), L.ptr(tq), L.ptr(tc),
                   L.ptr(pos), float(T), float(ce_w), float(kd_w), float(alpha), float(beta), *scale_slots, L.ptr(scores),
                   L.ptr(tscores), *outs)
        ctx.save_for_backward(dq, dc)
        return losses[0], losses.detach()

    @staticmethod
    def backward(ctx, g, g_all):
        dq, dc = ctx.saved_tensors
        return (dq * g, dc * g) + (None,) * 7


def _slots(q_vectors, ctx_vectors, local_q, local_ctx):
    """(q_lo, q_n, c_lo, c_n): the rows that carry gradient; default all rows."""
    q_lo, q_n = local_q if local_q is not None else (0, q_vectors.shape[0])
    c_lo, c_n = local_ctx if local_ctx is not None else (0, ctx_vectors.shape[0])
    return q_lo, q_n, c_lo, c_n


def inbatch_nll_loss(q_vectors, ctx_vectors, positive_idx_per_question, loss_scale=None, local_q=None, local_ctx=None):
    """dot_product_scores + log_softmax + nll_loss(mean) + argmax count (models.py:468-505).
    local_q / local_ctx = (lo, n): rows that carry gradient (multi-GPU gather semantics,
    PROD/ProD_base/train_DE_model_marco.py:251-264); default all rows."""
    loss, allv = _ScoresFn.apply(q_vectors, ctx_vectors, positive_idx_per_question, loss_scale,
                                 *_slots(q_vectors, ctx_vectors, local_q, local_ctx), None)
    return loss, allv[3]


def bi_kd_loss(q_vectors, ctx_vectors, teacher_q_vector, teacher_ctxs_vector, positive_idx_per_question, temperature=4.0,
               ce_weight=0.1, kd_weight=0.9, loss_scale=None, local_q=None, local_ctx=None, kd_type="KD_softmax",
               dkd_alpha=None, dkd_beta=None):
    """BiEncoderKDLoss.calc (PROD/ProD_KD/model/models.py:970-1038): all-pairs scores of the student and of the (constant)
    teacher embeddings, soft term chosen by ``kd_type`` (KD_softmax, KD_logit, DKD with ``dkd_alpha`` / ``dkd_beta``), or
    Bi_logit: an MSE between student and teacher embeddings of the same width.  -> (loss, hard, soft, correct_count)."""
    kd, alpha, beta = _kd_kind(BI_KD_TYPES, kd_type, dkd_alpha, dkd_beta)
    loss, allv = _ScoresFn.apply(q_vectors, ctx_vectors, positive_idx_per_question, loss_scale,
                                 *_slots(q_vectors, ctx_vectors, local_q, local_ctx),
                                 (kd, teacher_q_vector, teacher_ctxs_vector, temperature, ce_weight, kd_weight, alpha, beta))
    return loss, allv[1], allv[2], allv[3]


def fused_normal_inbatch_loss(q, ctx_vectors, reranker_logits, positive_idx_per_question, global_q=None, global_ctx=None,
                              local_q=None, local_ctx=None, temperature_normal=1.0, inbatch_weight=0.2, grad_accum=1,
                              scale_simmila=False):
    """L5, MASTER/finetune/MS/co_training_model.py:249-270: AR2 normal loss (L2 with lambda = 0) on the local block
    + inbatch_weight * BiEncoderNllLoss on the (gathered) all-pairs scores.  -> (loss, normal_loss, nll_loss, correct)."""
    loss_n, normal, _, _ = wiki_normal_adv_loss(q, ctx_vectors, reranker_logits, temperature_normal, 0.0, scale_simmila, grad_accum)
    gq = q if global_q is None else global_q
    gc = ctx_vectors if global_ctx is None else global_ctx
    nll, correct = inbatch_nll_loss(gq, gc, positive_idx_per_question, None, local_q, local_ctx)
    return loss_n + inbatch_weight * nll / grad_accum, normal, nll, correct


# ------------------------------------------------------------------------------------------ L7 (LEAD)
class _LeadScoresFn(torch.autograd.Function):
    """simx_lead_scores_fwd_bwd: n slots of student / teacher all-pairs scores, gradients for all four inputs."""

    @staticmethod
    def forward(ctx, q, c, tq, tc, pos_idx, slots, T, LT, teacher_grad, loss_scale, q_lo, q_n, c_lo, c_n):
        q, c, tq, tc = _f32c(q), _f32c(c), _f32c(tq), _f32c(tc)
        n, Q, H = q.shape
        Cn, HT = c.shape[1], tq.shape[2]
        dev = q.device
        pos = torch.as_tensor(pos_idx, dtype=torch.int32, device=dev).contiguous()
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        scores, tscores, slot_losses, weights, total = e(n, Q, Cn), e(n, Q, Cn), e(n, 4), e(n), e(1)
        dq, dc = e(n, q_n, H), e(n, c_n, H)
        dtq, dtc = (e(n, q_n, HT), e(n, c_n, HT)) if teacher_grad else (None, None)
        wsb = int(L.load().simx_lead_scores_workspace_bytes(n, Q, Cn, H, HT, q_n, c_n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        L.call("simx_lead_scores_fwd_bwd", L.stream_ptr(), n, Q, Cn, H, HT, L.ptr(q), L.ptr(c), L.ptr(tq), L.ptr(tc), L.ptr(pos),
               float(T), float(LT), slots, int(bool(teacher_grad)), float(loss_scale or 1.0), q_lo, q_n, c_lo, c_n,
               L.ptr(scores), L.ptr(tscores), L.ptr(slot_losses), L.ptr(weights), L.ptr(total), L.ptr(dq), L.ptr(dc),
               L.ptr(dtq), L.ptr(dtc), L.ptr(ws), wsb)
        ctx.slots_lo = (q_lo, Q, c_lo, Cn)
        ctx.save_for_backward(*(t for t in (dq, dc, dtq, dtc) if t is not None))
        ctx.mark_non_differentiable(slot_losses, weights)
        return total[0], slot_losses, weights

    @staticmethod
    def backward(ctx, g, g_slots, g_weights):
        q_lo, Q, c_lo, Cn = ctx.slots_lo

        def full(d, lo, rows):                          # the local rows' gradient inside the gathered tensor's
            if d.shape[1] == rows:
                return d * g
            out = torch.zeros(d.shape[0], rows, d.shape[2], dtype=d.dtype, device=d.device)
            out[:, lo:lo + d.shape[1]] = d * g
            return out
        saved = ctx.saved_tensors
        dq, dc = full(saved[0], q_lo, Q), full(saved[1], c_lo, Cn)
        dtq, dtc = (full(saved[2], q_lo, Q), full(saved[3], c_lo, Cn)) if len(saved) == 4 else (None, None)
        return (dq, dc, dtq, dtc) + (None,) * 10


def lead_layer_score_loss(q, ctx, tq, tctx, positive_idx, slots, temperature, layer_temperature, teacher_grad=True,
                          loss_scale=None, local_q=None, local_ctx=None):
    """The slot objective of LEAD's distill_loss (LEAD/util.py:540-831; simx_lead_scores_fwd_bwd in include/simx.h) in one call:
    q [n,Q,H], ctx [n,C,H] the student's and tq [n,Q,HT], tctx [n,C,HT] the teacher's vectors of n slots; ``slots`` a list of
    n (a, b, w, x, reweight) = the weights of nll_s, nll_t, kl_ts, kl_st and whether w is the layer-score softmax weight.
    -> (total, slot_losses [n,4], weights [n]); only ``total`` is differentiable, towards the teacher only with
    ``teacher_grad``.  local_q / local_ctx = (lo, n): the rows that carry gradient, as in inbatch_nll_loss."""
    if q.dim() != 3 or ctx.dim() != 3 or tq.dim() != 3 or tctx.dim() != 3:
        raise ValueError("lead_layer_score_loss: q, ctx, tq, tctx must be [n, rows, width]")
    n = q.shape[0]
    if not (ctx.shape[0] == tq.shape[0] == tctx.shape[0] == n and tq.shape[1] == q.shape[1] and tctx.shape[1] == ctx.shape[1]
            and ctx.shape[2] == q.shape[2] and tctx.shape[2] == tq.shape[2]):
        raise ValueError("lead_layer_score_loss: shapes %s %s %s %s do not form n slots of Q x C scores"
                         % (tuple(q.shape), tuple(ctx.shape), tuple(tq.shape), tuple(tctx.shape)))
    if len(slots) != n or not 1 <= n <= L.LEAD_MAX_SLOTS:
        raise ValueError("lead_layer_score_loss: %d slot weights for %d slots (1..%d)" % (len(slots), n, L.LEAD_MAX_SLOTS))
    arr = (L.LeadSlot * n)(*[L.LeadSlot(float(a), float(b), float(w), float(x), int(bool(rw))) for a, b, w, x, rw in slots])
    q_lo, q_n, c_lo, c_n = _slots(q[0], ctx[0], local_q, local_ctx)
    if not teacher_grad:
        tq, tctx = tq.detach(), tctx.detach()
    return _LeadScoresFn.apply(q, ctx, tq, tctx, positive_idx, arr, temperature, layer_temperature, bool(teacher_grad), loss_scale,
                               q_lo, q_n, c_lo, c_n)


def dot_product_scores(q_vectors, ctx_vectors):
    """q @ ctx^T on the strided f32 GEMM kernel (no grad; the training path uses inbatch_nll_loss)."""
    q, c = _f32c(q_vectors.detach()), _f32c(ctx_vectors.detach())
    out = torch.empty(q.shape[0], c.shape[0], dtype=torch.float32, device=q.device)
    H = q.shape[1]
    L.call("simx_gemm_f32_strided", L.stream_ptr(), q.shape[0], c.shape[0], H, L.ptr(q), H, 1, L.ptr(c), 1, H,
           L.ptr(out), c.shape[0], 0)
    return out


# ------------------------------------------------------------------------------------------ small linear (Reranker head)
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _f32c(x), _f32c(w)
        n, H = x.shape
        O = w.shape[0]
        y = torch.empty(n, O, dtype=torch.float32, device=x.device)
        L.call("simx_gemm_f32_strided", L.stream_ptr(), n, O, H, L.ptr(x), H, 1, L.ptr(w), 1, H, L.ptr(y), O, 0)
        if b is not None:
            y += b
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32c(dy)
        n, H = x.shape
        O = w.shape[0]
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        s = L.stream_ptr()
        L.call("simx_gemm_f32_strided", s, n, H, O, L.ptr(dy), O, 1, L.ptr(w), H, 1, L.ptr(dx), H, 0)
        L.call("simx_gemm_f32_strided", s, O, H, n, L.ptr(dy), 1, O, L.ptr(x), H, 1, L.ptr(dw), H, 0)
        db = None
        if ctx.has_b:
            db = torch.empty(O, dtype=torch.float32, device=x.device)
            L.call("simx_colsum", s, L.SIMX_F32, n, O, L.ptr(dy), O, L.ptr(db), 0)
        return dx, dw, db


def linear_f32(x, weight, bias=None):
    return _LinearFn.apply(x, weight, bias)


# ------------------------------------------------------------------------------------------ sampler
LAPLACE, GAUSS = 0, 1


def simans_sample(scores, pos_score, num_neg, form=LAPLACE, a=0.5, b=0.0, tau=3.0, seed=0, offset=0,
                  return_union=False, return_weights=False):
    """On-GPU SimANS draw.  scores [nq,C] f64 (rank order), pos_score [nq] f64 -> neg indices [nq,N] int32."""
    if not scores.is_cuda:
        raise L.SimxError("simans_sample runs only on a HIP device")
    scores = scores.contiguous().to(torch.float64)
    pos_score = pos_score.contiguous().to(torch.float64)
    nq, Cn = scores.shape
    dev = scores.device
    neg = torch.empty(nq, num_neg, dtype=torch.int32, device=dev)
    uni = torch.full((nq, 2 * num_neg), -1, dtype=torch.int32, device=dev) if return_union else None
    cnt = torch.zeros(nq, dtype=torch.int32, device=dev) if return_union else None
    wts = torch.empty(nq, Cn, dtype=torch.float64, device=dev) if return_weights else None
    L.call("simx_simans_sample", L.stream_ptr(), nq, Cn, num_neg, L.ptr(scores), L.ptr(pos_score), int(form),
           float(a), float(b), float(tau), C.c_uint64(int(seed)), C.c_uint32(int(offset)), L.ptr(neg), L.ptr(uni),
           L.ptr(cnt), L.ptr(wts))
    out = (neg,)
    if return_union:
        out += (uni, cnt)
    if return_weights:
        out += (wts,)
    return out if len(out) > 1 else neg


# ------------------------------------------------------------------------------------------ mined-negative pool
def mine_negatives(D, I, pos_ptr, pos_ids, top=200, want_negatives=True):
    """A search result D, I [nq,k] (f32 scores, int64 ids, rows sorted, (-inf, -1) padding at the tail) against the CSR of each
    query's positives (pos_ptr int32 [nq+1], pos_ids int64, in the id space of I) -> dict of device tensors: ``pos_scores``
    f32 [len(pos_ids)] (0 where the positive is not among the first ``top`` valid ranks), ``first_hit`` int32 [nq] (1 + the first
    rank of a positive over all k columns, 0 = none) and, with ``want_negatives``, ``neg_rows`` int32 / ``neg_scores`` f32
    [nq,top] (the non-positives of the first ``top`` valid ranks, rank order, right-aligned behind (0, +inf) padding) and
    ``neg_cnt`` int32 [nq].  Semantics and requirements: simx_mine_negatives (include/simx.h)."""
    for t in (D, I, pos_ptr, pos_ids):
        if not t.is_cuda:
            raise L.SimxError("mine_negatives runs only on a HIP device (no CPU fallback)")
    if D.dim() != 2 or D.shape != I.shape:
        raise ValueError("mine_negatives: D and I must be [nq, k] of one shape, got %s and %s" % (tuple(D.shape), tuple(I.shape)))
    nq, k = D.shape
    dev = D.device
    D = D.contiguous().to(torch.float32)
    I = I.contiguous().to(torch.int64)
    pos_ptr = pos_ptr.contiguous().to(torch.int32)
    pos_ids = pos_ids.contiguous().to(torch.int64)
    if pos_ptr.numel() != nq + 1 or int(pos_ptr[-1]) != pos_ids.numel():
        raise ValueError("mine_negatives: pos_ptr must hold nq + 1 = %d offsets ending at len(pos_ids) = %d" % (nq + 1, pos_ids.numel()))
    top = int(top)
    out = {"pos_scores": torch.empty(pos_ids.numel(), dtype=torch.float32, device=dev),
           "first_hit": torch.empty(nq, dtype=torch.int32, device=dev)}
    if want_negatives:
        out["neg_rows"] = torch.empty(nq, max(top, 0), dtype=torch.int32, device=dev)
        out["neg_scores"] = torch.empty(nq, max(top, 0), dtype=torch.float32, device=dev)
        out["neg_cnt"] = torch.empty(nq, dtype=torch.int32, device=dev)
    L.call("simx_mine_negatives", L.stream_ptr(), nq, k, top, L.ptr(D), L.ptr(I), L.ptr(pos_ptr), L.ptr(pos_ids),
           L.ptr(out.get("neg_rows")), L.ptr(out.get("neg_scores")), L.ptr(out.get("neg_cnt")), L.ptr(out["pos_scores"]),
           L.ptr(out["first_hit"]))
    return out


# ------------------------------------------------------------------------------------------ D1
def assemble_batch(q_tok, p_tok, q_rows, p_rows, docs_per_question, pad_id=0, sep_id=102, ce_len=160):
    """Device-side collate (MARCO_until_new.py:204-258) on pre-tokenised int32 tables in HBM.
    -> dict(student=[q_ids, q_mask, ctx_ids, ctx_mask, positive_ctx_indices], teacher=[ce_ids, ce_mask, tgt], lens=...)
    with the reference's shapes/dtypes ([B,QL], [B*D,PL], [B,D,CL] int64)."""
    assert q_tok.dtype == torch.int32 and p_tok.dtype == torch.int32 and q_tok.is_contiguous() and p_tok.is_contiguous()
    dev = q_tok.device
    q_rows = torch.as_tensor(q_rows, dtype=torch.int32, device=dev).contiguous()
    p_rows = torch.as_tensor(p_rows, dtype=torch.int32, device=dev).contiguous().view(-1)
    B, D = q_rows.numel(), int(docs_per_question)
    assert p_rows.numel() == B * D
    QL, PL = q_tok.shape[1], p_tok.shape[1]
    e = lambda *sh: torch.empty(*sh, dtype=torch.int64, device=dev)
    q_ids, q_mask, c_ids, c_mask = e(B, QL), e(B, QL), e(B * D, PL), e(B * D, PL)
    ce_ids, ce_mask = e(B, D, ce_len), e(B, D, ce_len)
    ql = torch.empty(B, dtype=torch.int32, device=dev)
    cl = torch.empty(B * D, dtype=torch.int32, device=dev)
    cel = torch.empty(B * D, dtype=torch.int32, device=dev)
    L.call("simx_assemble_batch", L.stream_ptr(), B, D, QL, PL, ce_len, L.ptr(q_tok), L.ptr(p_tok), L.ptr(q_rows), L.ptr(p_rows),
           int(pad_id), int(sep_id), L.ptr(q_ids), L.ptr(q_mask), L.ptr(c_ids), L.ptr(c_mask), L.ptr(ce_ids), L.ptr(ce_mask),
           L.ptr(ql), L.ptr(cl), L.ptr(cel))
    pos = [i * D for i in range(B)]
    tgt = torch.zeros(B, D, dtype=torch.int64, device=dev)
    tgt[:, 0] = 1
    return {"student": [q_ids, q_mask, c_ids, c_mask, pos], "teacher": [ce_ids, ce_mask, tgt],
            "lens": {"q": ql, "ctx": cl, "ce": cel}}


# ------------------------------------------------------------------------------------------ small f32 LayerNorm (E4 head)
class _LnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x, w, b = _f32c(x), _f32c(weight), _f32c(bias)
        T, H = x.shape
        y = torch.empty_like(x)
        L.call("simx_ln_fwd", L.stream_ptr(), L.SIMX_F32, T, H, L.ptr(x), L.ptr(w), L.ptr(b), float(eps), L.ptr(y))
        ctx.save_for_backward(x, w)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32c(dy)
        T, H = x.shape
        dx = torch.empty_like(x)
        dg = torch.zeros(H, dtype=torch.float32, device=x.device)
        db = torch.zeros(H, dtype=torch.float32, device=x.device)
        L.call("simx_ln_bwd", L.stream_ptr(), L.SIMX_F32, T, H, L.ptr(x), L.ptr(w), ctx.eps, L.ptr(dy), L.ptr(dx), L.ptr(dg), L.ptr(db), None)
        return dx, dg, db, None


def layer_norm_f32(x, weight, bias, eps=1e-5):
    """nn.LayerNorm on [n,H] f32 rows through simx_ln_fwd / simx_ln_bwd (H % 4 == 0, H <= 1024)."""
    return _LnFn.apply(x, weight, bias, eps)
