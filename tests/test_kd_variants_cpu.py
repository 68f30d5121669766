"""The KD_type objectives of CrossBERTKDLoss / BiEncoderKDLoss (PROD/ProD_KD/model/models.py:668-827, 970-1113) without a GPU:
(a) a float64 NumPy restatement of their formulas, written here, against tests/golden/losses_kd_variants.npz (the imported
reference's autograd, tools/make_kd_golden.py) to 1e-11 -- this pins what the golden means, and tests/test_kd_variants_gpu.py
checks the kernels against the same restatement on other shapes; (b) the argument errors, raised before any device access."""
import os
import types

import numpy as np
import pytest

CROSS_TYPES = ("KD_softmax", "KD_logit", "DKD", "prob_loss")
BI_TYPES = ("KD_softmax", "KD_logit", "DKD", "Bi_logit")


# ------------------------------------------------------------------------------------------ the restatement (float64)
def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _log_softmax(x):
    x = x - x.max(1, keepdims=True)
    return x - np.log(np.exp(x).sum(1, keepdims=True))


def _kl_rows(u, log_u, log_p):
    """sum_c u (log u - log p) per row with 0 log 0 = 0 (F.kl_div)."""
    return np.where(u > 0, u * (log_u - log_p), 0.0).sum(1)


def hard_term(S, pos):
    """NLL(log_softmax(S), pos) averaged over the rows -> (hard, correct count, d hard / dS)."""
    n = S.shape[0]
    rows = np.arange(n)
    onehot = np.zeros_like(S)
    onehot[rows, pos] = 1.0
    hard = -_log_softmax(S)[rows, pos].mean()
    correct = int((S.argmax(1) == pos).sum())           # first maximum, as torch.max
    return hard, correct, (_softmax(S) - onehot) / n


def soft_term(kd_type, S, Z, pos, T, alpha=None, beta=None):
    """-> (soft, d soft / dS) of one KD_type on student scores S and teacher scores Z [n, m], target column pos[i]."""
    n, m = S.shape
    if kd_type == "KD_softmax":                         # T^2 * mean_rows KL(softmax(Z/T) || softmax(S/T))
        u = _softmax(Z / T)
        return T * T * _kl_rows(u, np.log(np.where(u > 0, u, 1.0)), _log_softmax(S / T)).mean(), (T / n) * (_softmax(S / T) - u)
    if kd_type == "KD_logit":                           # 0.5 * mean over all n*m elements of (S - Z)^2; T is not used
        return 0.5 * ((S - Z) ** 2).mean(), (S - Z) / (n * m)
    if kd_type == "prob_loss":                          # -(1/n) sum softmax(Z/T) log(softmax(S) + 1e-7)
        eps = 1e-7
        u, p = _softmax(Z / T), _softmax(S)
        g = -u / (n * (p + eps))
        return -(u * np.log(p + eps)).sum() / n, p * (g - (g * p).sum(1, keepdims=True))
    assert kd_type == "DKD"
    rows = np.arange(n)
    gt = np.zeros_like(S)
    gt[rows, pos] = 1.0
    p, u = _softmax(S / T), _softmax(Z / T)
    p_gt, u_gt = (p * gt).sum(1), (u * gt).sum(1)
    p_o, u_o = (p * (1 - gt)).sum(1), (u * (1 - gt)).sum(1)          # sums over the other columns, not 1 - p_gt
    xlogy = lambda a, b: np.where(a > 0, a * (np.log(np.where(a > 0, a, 1.0)) - np.log(b)), 0.0)
    tckd = (T * T / n) * (xlogy(u_gt, p_gt) + xlogy(u_o, p_o)).sum()
    pm, um = _softmax(S / T - 1000.0 * gt), _softmax(Z / T - 1000.0 * gt)
    nckd = (T * T / n) * _kl_rows(um, np.log(np.where(um > 0, um, 1.0)), _log_softmax(S / T - 1000.0 * gt)).sum()
    d_tckd = (T / n) * np.where(gt > 0, p - u, p * ((p_o - u_o) / p_o)[:, None])
    d_nckd = (T / n) * (pm - um)
    return alpha * tckd + beta * nckd, alpha * d_tckd + beta * d_nckd


def cross_ref(q, c, z, kd_type, T, ce_w, kd_w, alpha=None, beta=None, lwf=None, lwf_w=0.0):
    """CrossBERTKDLoss.calc: q [B,H], c [B*D,H], teacher logits z [B,D], positive at column 0; lwf = (qo, co) of the frozen
    student.  -> (loss, correct, dq, dc)."""
    B, H = q.shape
    c3 = c.reshape(B, -1, H)
    S = np.einsum("bh,bdh->bd", q, c3)
    pos = np.zeros(B, dtype=np.int64)
    hard, correct, dS = hard_term(S, pos)
    soft, dsoft = soft_term(kd_type, S, z, pos, T, alpha, beta)
    loss, dS = ce_w * hard + kd_w * soft, ce_w * dS + kd_w * dsoft
    if lwf is not None:
        So = np.einsum("bh,bdh->bd", lwf[0], lwf[1].reshape(B, -1, H))
        l2, d2 = soft_term(kd_type, S, So, pos, T)
        loss, dS = loss + lwf_w * l2, dS + lwf_w * d2
    return loss, correct, np.einsum("bd,bdh->bh", dS, c3), (dS[:, :, None] * q[:, None, :]).reshape(c.shape)


def bi_ref(q, c, tq, tc, pos, kd_type, T, ce_w, kd_w, alpha=None, beta=None, loss_scale=1.0):
    """BiEncoderKDLoss.calc on the gathered q [Q,H], c [C,H] and teacher embeddings -> (loss, correct, dq, dc), gradients for
    every row (a rank keeps the rows of its own slot)."""
    pos = np.asarray(pos, dtype=np.int64)
    S = q @ c.T
    hard, correct, dS = hard_term(S, pos)
    dq_x, dc_x = 0.0, 0.0
    if kd_type == "Bi_logit":                           # 0.5 * MSE(q, tq) + 0.5 * MSE(c, tc) on the embeddings
        soft = 0.5 * ((q - tq) ** 2).mean() + 0.5 * ((c - tc) ** 2).mean()
        dq_x, dc_x = kd_w * (q - tq) / q.size, kd_w * (c - tc) / c.size
        dS = ce_w * dS
    else:
        soft, dsoft = soft_term(kd_type, S, tq @ tc.T, pos, T, alpha, beta)
        dS = ce_w * dS + kd_w * dsoft
    loss = ce_w * hard + kd_w * soft
    return loss_scale * loss, correct, loss_scale * (dS @ c + dq_x), loss_scale * (dS.T @ q + dc_x)


# ------------------------------------------------------------------------------------------ (a) restatement == golden
@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "losses_kd_variants.npz"))


def _hp(G):
    return dict(T=float(G["T"]), ce_w=float(G["CE_WEIGHT"]), kd_w=float(G["KD_WEIGHT"]), alpha=float(G["DKD_alpha"]),
                beta=float(G["DKD_beta"]))


def _same(G, key, got, tol=1e-11):
    loss, correct, dq, dc = got
    for what, v in (("loss", loss), ("dq", dq), ("dc", dc)):
        ref = G["%s.%s" % (key, what)]
        err = np.abs(np.asarray(v) - ref).max()
        assert err <= tol * max(1.0, np.abs(ref).max()), "%s.%s: err %.3e" % (key, what, err)
    assert correct == int(G[key + ".correct"]), key


def test_golden_has_the_required_cases(G):
    assert (float(G["T"]), float(G["CE_WEIGHT"]), float(G["KD_WEIGHT"]), float(G["DKD_alpha"]), float(G["DKD_beta"])) == (4.0, 0.1, 0.9, 1.0, 8.0)
    pos = G["b_pos"]
    assert 0 in pos and G["b_c"].shape[0] - 1 in pos
    assert G["b_tq"].shape[1] != G["b_q"].shape[1]
    for fam, n in (("cross.DKD", G["x_q"].shape[0]), ("bi.DKD", G["b_q"].shape[0])):
        assert 0 < int(G[fam + ".correct"]) < n         # a correctly and a wrongly classified row
    assert all(np.isfinite(G[k]).all() for k in G.files)


@pytest.mark.parametrize("name", CROSS_TYPES + ("KD_logit_lwf",))
def test_restatement_matches_reference_cross(G, name):
    f = lambda k: G[k].astype(np.float64)
    kd_type = "KD_logit" if name == "KD_logit_lwf" else name
    lwf = (f("x_qo"), f("x_co")) if name == "KD_logit_lwf" else None
    _same(G, "cross." + name, cross_ref(f("x_q"), f("x_c"), f("x_z"), kd_type, lwf=lwf, lwf_w=float(G["LwF_WEIGHT"]), **_hp(G)))


@pytest.mark.parametrize("kd_type", BI_TYPES)
def test_restatement_matches_reference_bi(G, kd_type):
    f = lambda k: G[k].astype(np.float64)
    tq, tc = (f("b_tqh"), f("b_tch")) if kd_type == "Bi_logit" else (f("b_tq"), f("b_tc"))
    _same(G, "bi." + kd_type, bi_ref(f("b_q"), f("b_c"), tq, tc, G["b_pos"], kd_type, **_hp(G)))


def dist_inputs(G, kd_type, W=2):
    """The gathered W = 2 batch of the dist.* cases: (q, c, tq, tc, pos, [(q_lo, q_n)], [(c_lo, c_n)])."""
    f = lambda k: G[k].astype(np.float64)
    tqk, tck = ("d_tqh%d", "d_tch%d") if kd_type == "Bi_logit" else ("d_tq%d", "d_tc%d")
    cat = lambda k: np.concatenate([f(k % r) for r in range(W)], 0)
    nq, nc = G["d_q0"].shape[0], G["d_c0"].shape[0]
    return (cat("d_q%d"), cat("d_c%d"), cat(tqk), cat(tck), G["d_pos"], [(r * nq, nq) for r in range(W)],
            [(r * nc, nc) for r in range(W)])


@pytest.mark.parametrize("kd_type", BI_TYPES[1:])
def test_restatement_matches_reference_gathered(G, kd_type):
    q, c, tq, tc, pos, qs, cs = dist_inputs(G, kd_type)
    loss, correct, dq, dc = bi_ref(q, c, tq, tc, pos, kd_type, loss_scale=float(G["dist_loss_scale"]), **_hp(G))
    for r, ((q_lo, q_n), (c_lo, c_n)) in enumerate(zip(qs, cs)):
        _same(G, "dist.%s.r%d" % (kd_type, r), (loss, correct, dq[q_lo:q_lo + q_n], dc[c_lo:c_lo + c_n]))


def test_restatement_gradients_are_the_derivative():
    """The closed forms of soft_term against central differences of its own value (float64)."""
    rs = np.random.RandomState(5)
    S, Z, pos = rs.randn(3, 7) * 2, rs.randn(3, 7) * 2, np.array([0, 6, 3])
    for kd_type in CROSS_TYPES:
        _, d = soft_term(kd_type, S, Z, pos, 4.0, 1.0, 8.0)
        num = np.zeros_like(S)
        for i in np.ndindex(*S.shape):
            e = np.zeros_like(S)
            e[i] = 1e-6
            num[i] = (soft_term(kd_type, S + e, Z, pos, 4.0, 1.0, 8.0)[0] - soft_term(kd_type, S - e, Z, pos, 4.0, 1.0, 8.0)[0]) / 2e-6
        assert np.abs(num - d).max() <= 1e-8, kd_type


# ------------------------------------------------------------------------------------------ (b) argument errors
class _NoDevice(object):
    """Stands in for a tensor: any use of it is a failure of 'validate before any device work'."""

    def __getattr__(self, name):
        raise AssertionError("the loss touched its tensors (.%s) before validating the arguments" % name)


def _ns(**kw):
    base = dict(TEMPERATURE=4.0, CE_WEIGHT=0.1, KD_WEIGHT=0.9, LwF_WEIGHT=1.0, DKD_alpha=1.0, DKD_beta=8.0)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("cls,args,lwf,flag", [
    ("cross", _ns(KD_type="KD_sofmax"), False, "KD_type"),
    ("bi", _ns(KD_type="nope"), False, "KD_type"),
    ("bi", _ns(KD_type="prob_loss"), False, "KD_type"),
    ("cross", _ns(KD_type="Bi_logit"), False, "KD_type"),
    ("cross", _ns(KD_type="DKD", DKD_alpha=None), False, "DKD_alpha"),
    ("cross", _ns(KD_type="DKD", DKD_beta=None), False, "DKD_beta"),
    ("bi", _ns(KD_type="DKD", DKD_alpha=None), False, "DKD_alpha"),
    ("bi", types.SimpleNamespace(KD_type="DKD", TEMPERATURE=4.0, CE_WEIGHT=0.1, KD_WEIGHT=0.9), False, "DKD_beta"),
    ("cross", _ns(KD_type="DKD"), True, "KD_type"),
    ("cross", _ns(KD_type="prob_loss"), True, "KD_type"),
])
def test_bad_arguments_raise_value_error_before_device_work(cls, args, lwf, flag):
    from simxns_amd.model.models import BiEncoderKDLoss, CrossBERTKDLoss
    t = _NoDevice()
    with pytest.raises(ValueError) as ei:
        if cls == "cross":
            CrossBERTKDLoss().calc(args, t, t, t, LwF=lwf, ori_q_vector=t, ori_ctx_vectors=t)
        else:
            BiEncoderKDLoss().calc(args, t, t, t, t, [0])
    assert flag in str(ei.value)


def test_ops_reject_bad_kd_type_before_device_work():
    from simxns_amd import ops
    t = _NoDevice()
    with pytest.raises(ValueError):
        ops.cross_kd_loss(t, t, t, kd_type="Bi_logit")
    with pytest.raises(ValueError):
        ops.bi_kd_loss(t, t, t, t, [0], kd_type="prob_loss")
    with pytest.raises(ValueError):
        ops.bi_kd_loss(t, t, t, t, [0], kd_type="DKD", dkd_alpha=1.0)


def test_loss_params_struct_matches_header():
    """simx_loss_params grew at its end: the ctypes mirror has the header's fields in the header's order."""
    import re
    from simxns_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "simx.h")).read()
    body = re.search(r"typedef struct simx_loss_params \{(.*?)\} simx_loss_params;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.LossParams._fields_]
    assert names[:7] == ["kind", "scale", "temperature", "adv_lambda", "ce_w", "kd_w", "grad_accum"]
