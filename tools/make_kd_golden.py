"""Write tests/golden/losses_kd_variants.npz: every KD_type objective of the PROD loss classes, computed by the IMPORTED
REFERENCE (PROD/ProD_KD/model/models.py: CrossBERTKDLoss, BiEncoderKDLoss) in float64 with torch autograd.

TEST INFRASTRUCTURE, the companion of oracle/make_golden.py::gen_losses for the objectives that file does not drive; it
needs a checkout of the reference project (not needed to build, test or run the package), only the .npz travels.
Run:  python -m tools.make_kd_golden [--reference DIR]

Per case the file holds loss, correct, dq, dc (keys "<family>.<case>.<what>"), next to the inputs:
  cross.<KD_type>            CrossBERTKDLoss on x_q [B,H], x_c [B*D,H], teacher logits x_z [B,D]
  cross.KD_logit_lwf         the same with LwF=True against the frozen student's x_qo, x_co
  bi.<KD_type>               BiEncoderKDLoss on b_q [Q,H], b_c [C,H], positives b_pos, teacher b_tq / b_tc [.,HT] (HT != H;
                             Bi_logit: b_tqh / b_tch [.,H])
  dist.<KD_type>.r<rank>     the gathered W = 2 batch as rank r sees it (only its own d_q<r> / d_c<r> carry gradient, built
                             like dist_* of losses.npz), loss_scale = 2
Inputs are rounded to float32 first (and stored so), so the engine's f32 kernels see exactly the numbers the reference saw;
alpha = 1 and beta = 8 are both non-zero, so a finite DKD loss means both of its terms are finite.
"""
import argparse
import os
import types
import warnings

import numpy as np
import torch

from oracle.make_golden import REF, _load

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "losses_kd_variants.npz")
T, CE_W, KD_W, ALPHA, BETA, LWF_W, DIST_SCALE = 4.0, 0.1, 0.9, 1.0, 8.0, 1.0, 2.0
CROSS_TYPES = ("KD_softmax", "KD_logit", "DKD", "prob_loss")
BI_TYPES = ("KD_softmax", "KD_logit", "DKD", "Bi_logit")


def _args(kd_type):
    return types.SimpleNamespace(KD_type=kd_type, TEMPERATURE=T, CE_WEIGHT=CE_W, KD_WEIGHT=KD_W, LwF_WEIGHT=LWF_W,
                                 DKD_alpha=ALPHA, DKD_beta=BETA)


def _t(a, grad=False):
    return torch.tensor(a, dtype=torch.float64, requires_grad=grad)


def _put(out, key, loss, correct, dq, dc):
    vals = dict(loss=np.float64(loss.item()), correct=np.int64(int(correct)), dq=dq.grad.numpy().copy(), dc=dc.grad.numpy().copy())
    for k, v in vals.items():
        assert np.isfinite(v).all(), "%s.%s is not finite" % (key, k)
        out["%s.%s" % (key, k)] = v
    print(" %-22s loss %.12f correct %d |dq| %.3e |dc| %.3e" % (key, vals["loss"], vals["correct"], np.abs(vals["dq"]).max(),
                                                               np.abs(vals["dc"]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF, help="checkout of the reference project")
    ref = ap.parse_args().reference
    warnings.simplefilter("ignore")
    PR = _load("ref_prod_models", os.path.join(ref, "PROD/ProD_KD/model/models.py"))
    rs = np.random.RandomState(23)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    out = dict(T=T, CE_WEIGHT=CE_W, KD_WEIGHT=KD_W, DKD_alpha=ALPHA, DKD_beta=BETA, LwF_WEIGHT=LWF_W, dist_loss_scale=DIST_SCALE)

    # ---- CrossBERTKDLoss: [B, 1+N] block similarity, positive at column 0
    B, D, H = 6, 16, 32
    x = dict(x_q=f32(rs.randn(B, H) * 0.6), x_c=f32(rs.randn(B * D, H) * 0.6), x_z=f32(rs.randn(B, D) * 2.0),
             x_qo=f32(rs.randn(B, H) * 0.6), x_co=f32(rs.randn(B * D, H) * 0.6))
    x["x_c"][0::2 * D] = f32(x["x_c"][0::2 * D] + 0.8 * x["x_q"][0::2])     # every other query finds its positive
    out.update({k: v.astype(np.float32) for k, v in x.items()})
    sim = np.einsum("bh,bdh->bd", x["x_q"], x["x_c"].reshape(B, D, H))
    n_ok = int((sim.argmax(1) == 0).sum())
    assert 0 < n_ok < B, "the block case needs a correctly and a wrongly classified row (%d of %d correct)" % (n_ok, B)
    for name, kd_type, lwf in [(k, k, False) for k in CROSS_TYPES] + [("KD_logit_lwf", "KD_logit", True)]:
        q, c = _t(x["x_q"], True), _t(x["x_c"], True)
        loss, corr = PR.CrossBERTKDLoss().calc(_args(kd_type), q, c, _t(x["x_z"]), LwF=lwf, ori_q_vector=_t(x["x_qo"]),
                                               ori_ctx_vectors=_t(x["x_co"]))
        loss.backward()
        _put(out, "cross." + name, loss, corr, q, c)

    # ---- BiEncoderKDLoss: all-pairs scores, positives anywhere (column 0 and the last column included)
    Q, C, HT = 5, 20, 48
    pos = [0, 4, 8, 12, C - 1]
    b = dict(b_q=f32(rs.randn(Q, H) * 0.6), b_c=f32(rs.randn(C, H) * 0.6), b_tq=f32(rs.randn(Q, HT) * 0.5),
             b_tc=f32(rs.randn(C, HT) * 0.5), b_tqh=f32(rs.randn(Q, H) * 0.6), b_tch=f32(rs.randn(C, H) * 0.6))
    b["b_c"][pos[0::2]] = f32(b["b_c"][pos[0::2]] + 0.8 * b["b_q"][0::2])
    out.update({k: v.astype(np.float32) for k, v in b.items()}, b_pos=np.asarray(pos, dtype=np.int64))
    S = b["b_q"] @ b["b_c"].T
    n_ok = int((S.argmax(1) == np.asarray(pos)).sum())
    assert 0 < n_ok < Q, "the all-pairs case needs a correctly and a wrongly classified row (%d of %d correct)" % (n_ok, Q)
    for kd_type in BI_TYPES:
        q, c = _t(b["b_q"], True), _t(b["b_c"], True)
        tq, tc = (b["b_tqh"], b["b_tch"]) if kd_type == "Bi_logit" else (b["b_tq"], b["b_tc"])
        loss, corr = PR.BiEncoderKDLoss().calc(_args(kd_type), q, c, _t(tq), _t(tc), pos)
        loss.backward()
        _put(out, "bi." + kd_type, loss, corr, q, c)

    # ---- the gathered batch of W = 2 ranks: rank r's rows are leaves, the other rank's are constants
    W, Bq, Np = 2, 3, 4
    dpos = [j * Np for j in range(W * Bq)]
    dpos[-1] = W * Bq * Np - 1
    out["d_pos"] = np.asarray(dpos, dtype=np.int64)
    d = {}
    for r in range(W):
        d["d_q%d" % r], d["d_c%d" % r] = f32(rs.randn(Bq, H) * 0.6), f32(rs.randn(Bq * Np, H) * 0.6)
        d["d_tq%d" % r], d["d_tc%d" % r] = f32(rs.randn(Bq, HT) * 0.5), f32(rs.randn(Bq * Np, HT) * 0.5)
        d["d_tqh%d" % r], d["d_tch%d" % r] = f32(rs.randn(Bq, H) * 0.6), f32(rs.randn(Bq * Np, H) * 0.6)
    out.update({k: v.astype(np.float32) for k, v in d.items()})
    for kd_type in BI_TYPES[1:]:
        tqk, tck = ("d_tqh%d", "d_tch%d") if kd_type == "Bi_logit" else ("d_tq%d", "d_tc%d")
        tq = torch.cat([_t(d[tqk % i]) for i in range(W)], 0)
        tc = torch.cat([_t(d[tck % i]) for i in range(W)], 0)
        for r in range(W):
            lq, lc = _t(d["d_q%d" % r], True), _t(d["d_c%d" % r], True)
            gq = torch.cat([lq if i == r else _t(d["d_q%d" % i]) for i in range(W)], 0)
            gc = torch.cat([lc if i == r else _t(d["d_c%d" % i]) for i in range(W)], 0)
            loss, corr = PR.BiEncoderKDLoss().calc(_args(kd_type), gq, gc, tq, tc, dpos, loss_scale=DIST_SCALE)
            loss.backward()
            _put(out, "dist.%s.r%d" % (kd_type, r), loss, corr, lq, lc)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
