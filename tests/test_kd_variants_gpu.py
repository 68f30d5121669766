"""The KD_type objectives of CrossBERTKDLoss / BiEncoderKDLoss (KD_logit, DKD, prob_loss, Bi_logit) on the HIP kernels:
against the imported reference's float64 autograd (tests/golden/losses_kd_variants.npz) through the public classes, and
against the float64 restatement of tests/test_kd_variants_cpu.py on the shapes at which the kernels take another path.

Tolerance: the project's f32 loss bound, 3e-5 * max(1, |ref|_inf) (_close of tests/test_losses_sampler_gpu.py), for every
objective.  DKD's (p_o - u_o) / p_o term needs no more: the imported reference run on the CPU in float32 on the golden inputs
stays within 2.9e-7 (all-pairs DKD; block DKD 1.9e-7, the other objectives under 1e-7) of its own float64 result in the same
measure, a hundredth of the bound.  (The kernels on MI355X: at most 7e-7 on the golden cases, DKD's loss the largest.)"""
import hashlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from test_kd_variants_cpu import BI_TYPES, CROSS_TYPES, bi_ref, cross_ref, dist_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(T=4.0, ce_w=0.1, kd_w=0.9, alpha=1.0, beta=8.0)


def _close(got, ref, tol=3e-5, what=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max()
    lim = tol * max(1.0, np.abs(ref).max())
    print("%s: err %.3e (bound %.3e)" % (what, err, lim))
    assert err <= lim, "%s: err %.3e > %.3e" % (what, err, lim)


def _t(a, dev, req=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.requires_grad_(req)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _args(kd_type, **kw):
    a = dict(KD_type=kd_type, TEMPERATURE=HP["T"], CE_WEIGHT=HP["ce_w"], KD_WEIGHT=HP["kd_w"], LwF_WEIGHT=1.0,
             DKD_alpha=HP["alpha"], DKD_beta=HP["beta"])
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "losses_kd_variants.npz"))


# ------------------------------------------------------------------------------------------ golden parity, public classes
@pytest.mark.parametrize("name", CROSS_TYPES[1:] + ("KD_logit_lwf",))
def test_cross_kd_variants_golden(dev, G, name):
    from simxns_amd.model.models import CrossBERTKDLoss
    lwf = name == "KD_logit_lwf"
    tq, tc = _t(G["x_q"], dev, True), _t(G["x_c"], dev, True)
    loss, correct = CrossBERTKDLoss().calc(_args("KD_logit" if lwf else name), tq, tc, _t(G["x_z"], dev), LwF=lwf,
                                           ori_q_vector=_t(G["x_qo"], dev) if lwf else None,
                                           ori_ctx_vectors=_t(G["x_co"], dev) if lwf else None)
    loss.backward()
    key = "cross." + name
    _close(loss.item(), G[key + ".loss"], what=key + " loss")
    assert int(correct.item()) == int(G[key + ".correct"])
    _close(tq.grad.cpu().numpy(), G[key + ".dq"], what=key + " dq")
    _close(tc.grad.cpu().numpy(), G[key + ".dc"], what=key + " dc")


@pytest.mark.parametrize("kd_type", BI_TYPES[1:])
def test_bi_kd_variants_golden(dev, G, kd_type):
    from simxns_amd.model.models import BiEncoderKDLoss
    tq, tc = _t(G["b_q"], dev, True), _t(G["b_c"], dev, True)
    teach = ("b_tqh", "b_tch") if kd_type == "Bi_logit" else ("b_tq", "b_tc")
    loss, correct = BiEncoderKDLoss().calc(_args(kd_type), tq, tc, _t(G[teach[0]], dev), _t(G[teach[1]], dev),
                                           [int(v) for v in G["b_pos"]])
    loss.backward()
    key = "bi." + kd_type
    _close(loss.item(), G[key + ".loss"], what=key + " loss")
    assert int(correct.item()) == int(G[key + ".correct"])
    _close(tq.grad.cpu().numpy(), G[key + ".dq"], what=key + " dq")
    _close(tc.grad.cpu().numpy(), G[key + ".dc"], what=key + " dc")


@pytest.mark.parametrize("kd_type", BI_TYPES[1:])
def test_bi_kd_variants_gathered_golden(dev, G, kd_type):
    """The gathered batch as each of W = 2 ranks sees it: gradient on the local slot only, loss_scale = 2."""
    from simxns_amd.model.models import BiEncoderKDLoss
    q, c, tq_, tc_, pos, qs, cs = dist_inputs(G, kd_type)
    for r, (lq, lc) in enumerate(zip(qs, cs)):
        tq, tc = _t(q, dev, True), _t(c, dev, True)
        loss, correct = BiEncoderKDLoss().calc(_args(kd_type), tq, tc, _t(tq_, dev), _t(tc_, dev), [int(v) for v in pos],
                                               loss_scale=float(G["dist_loss_scale"]), local_q=lq, local_ctx=lc)
        loss.backward()
        key = "dist.%s.r%d" % (kd_type, r)
        _close(loss.item(), G[key + ".loss"], what=key + " loss")
        assert int(correct.item()) == int(G[key + ".correct"])
        gq, gc = tq.grad.cpu().numpy(), tc.grad.cpu().numpy()
        _close(gq[lq[0]:lq[0] + lq[1]], G[key + ".dq"], what=key + " dq")
        _close(gc[lc[0]:lc[0] + lc[1]], G[key + ".dc"], what=key + " dc")
        rest_q, rest_c = np.delete(gq, np.s_[lq[0]:lq[0] + lq[1]], 0), np.delete(gc, np.s_[lc[0]:lc[0] + lc[1]], 0)
        assert np.abs(rest_q).max() == 0.0 and np.abs(rest_c).max() == 0.0


# ------------------------------------------------------------------------------------------ shapes vs the restatement
def _emb(rs, n, H, spread=2.0):
    """Embeddings whose pairwise scores have a standard deviation of about ``spread``."""
    return _f32(rs.randn(n, H) * np.sqrt(spread / np.sqrt(H)))


@pytest.mark.parametrize("D", [2, 17, 64])
@pytest.mark.parametrize("kd_type", CROSS_TYPES[1:])
def test_cross_kd_variants_shapes(dev, kd_type, D):
    """Block form: B = 5 (a partial four-row block), D at both ends of the lane range and odd, H of one and of twelve strides."""
    from simxns_amd import ops
    B = 5
    for H in (64, 768):
        rs = np.random.RandomState(1000 * D + H)
        q, c, z = _emb(rs, B, H), _emb(rs, B * D, H), _f32(rs.randn(B, D) * 2.0)
        tq, tc = _t(q, dev, True), _t(c, dev, True)
        loss, correct, hard, soft = ops.cross_kd_loss(tq, tc, _t(z, dev), HP["T"], HP["ce_w"], HP["kd_w"], kd_type, HP["alpha"], HP["beta"])
        loss.backward()
        l, corr, dq, dc = cross_ref(q, c, z, kd_type, **HP)
        what = "%s D%d H%d " % (kd_type, D, H)
        _close(loss.item(), l, what=what + "loss")
        _close(HP["ce_w"] * hard.item() + HP["kd_w"] * soft.item(), l, what=what + "ce_w*hard + kd_w*soft")
        assert int(correct.item()) == corr
        _close(tq.grad.cpu().numpy(), dq, what=what + "dq")
        _close(tc.grad.cpu().numpy(), dc, what=what + "dc")


@pytest.mark.parametrize("C", [24, 130])
@pytest.mark.parametrize("kd_type", BI_TYPES[1:])
def test_bi_kd_variants_shapes(dev, kd_type, C):
    """All-pairs form: Q = 5 (a partial four-row block), C below one lane stride and with a tail after two, positives in the
    first and the last column, a local slot strictly inside the rows, loss_scale != 1, and a teacher of another width for the
    score-based types.  Bi_logit: rows outside the slot get exactly zero gradient and still count in the loss."""
    from simxns_amd import ops
    Q, H, scale = 5, 64, 3.0
    HT = H if kd_type == "Bi_logit" else 40
    rs = np.random.RandomState(C)
    q, c, tq_, tc_ = _emb(rs, Q, H), _emb(rs, C, H), _emb(rs, Q, HT), _emb(rs, C, HT)
    pos = [0, C // 3, C - 1, 64 % C, C // 2]
    lq, lc = (1, 3), (3, C - 8)
    tq, tc = _t(q, dev, True), _t(c, dev, True)
    loss, hard, soft, correct = ops.bi_kd_loss(tq, tc, _t(tq_, dev), _t(tc_, dev), pos, HP["T"], HP["ce_w"], HP["kd_w"], scale, lq, lc,
                                               kd_type, HP["alpha"], HP["beta"])
    loss.backward()
    l, corr, dq, dc = bi_ref(q, c, tq_, tc_, pos, kd_type, loss_scale=scale, **HP)
    what = "%s C%d " % (kd_type, C)
    _close(loss.item(), l, what=what + "loss")
    _close(scale * (HP["ce_w"] * hard.item() + HP["kd_w"] * soft.item()), l, what=what + "scale*(ce_w*hard + kd_w*soft)")
    assert int(correct.item()) == corr
    gq, gc = tq.grad.cpu().numpy(), tc.grad.cpu().numpy()
    _close(gq[1:4], dq[1:4], what=what + "dq local")
    _close(gc[3:C - 5], dc[3:C - 5], what=what + "dc local")
    assert np.abs(gq[:1]).max() == 0.0 and np.abs(gq[4:]).max() == 0.0
    assert np.abs(gc[:3]).max() == 0.0 and np.abs(gc[C - 5:]).max() == 0.0


def test_bi_logit_needs_equal_widths(dev):
    from simxns_amd import ops
    z = lambda n, h: torch.zeros(n, h, device=dev)
    with pytest.raises(ValueError):
        ops.bi_kd_loss(z(2, 64), z(4, 64), z(2, 32), z(4, 32), [0, 1], kd_type="Bi_logit")


def test_unknown_kind_is_unsupported(dev):
    """The C ABI itself: a loss kind / kd_type past the last one returns SIMX_ERR_UNSUPPORTED (-5) and launches nothing."""
    from simxns_amd import _lib as L, ops
    z = lambda *s: torch.zeros(*s, device=dev)
    q, c, t, sim, losses, dq, dc = z(2, 64), z(4, 64), z(2, 2), z(2, 2), z(4), z(2, 64), z(4, 64)
    lib = L.load()
    assert lib.simx_sim_loss_fwd_bwd(L.stream_ptr(), 2, 2, 64, L.ptr(q), L.ptr(c), L.ptr(t), ops._lp(7), L.ptr(sim), L.ptr(losses),
                                     L.ptr(dq), L.ptr(dc)) == -5
    pos = torch.zeros(2, dtype=torch.int32, device=dev)
    s, ts = z(2, 4), z(2, 4)
    assert lib.simx_scores_kd_type_fwd_bwd(L.stream_ptr(), 4, 2, 4, 64, 64, L.ptr(q), L.ptr(c), L.ptr(q), L.ptr(c), L.ptr(pos), 4.0, 0.1,
                                           0.9, 1.0, 8.0, 1.0, 0, 2, 0, 4, L.ptr(s), L.ptr(ts), L.ptr(losses), L.ptr(dq), L.ptr(dc),
                                           None, 0) == -5
    torch.cuda.synchronize()
    assert float(dq.abs().max()) == 0.0 and float(dc.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ one call, one row body
@pytest.mark.parametrize("rows", [2, 9])
def test_kd_softmax_defaulted_and_spelled_out_are_the_same_call(dev, rows):
    """KD_softmax with kd_type and the DKD weights spelled out == the call that leaves them at their defaults, bit for bit: both
    are the same launch, and alpha / beta reach no KD_softmax arithmetic.  The loss scalars are f32 atomic sums over the rows,
    whose order is only fixed for two rows (a + b == b + a), so they are compared there; the gradients and the per-row work
    carry no atomics and are compared at both sizes."""
    from simxns_amd import ops
    rs = np.random.RandomState(rows)
    D, H, C = 16, 64, 24
    q, c, z = _emb(rs, rows, H), _emb(rs, rows * D, H), _f32(rs.randn(rows, D) * 2.0)
    c2, tq_, tc_ = _emb(rs, C, H), _emb(rs, rows, 40), _emb(rs, C, 40)
    pos = [(5 * i) % C for i in range(rows)]

    def run(extra_pos, extra_kw):
        out = []
        tq, tc = _t(q, dev, True), _t(c, dev, True)
        res = ops.cross_kd_loss(tq, tc, _t(z, dev), 4.0, 0.1, 0.9, *extra_pos, **extra_kw)
        res[0].backward()
        out.append((res, tq.grad, tc.grad))
        tq, tc = _t(q, dev, True), _t(c2, dev, True)
        res = ops.bi_kd_loss(tq, tc, _t(tq_, dev), _t(tc_, dev), pos, 4.0, 0.1, 0.9, 2.0, None, None, *extra_pos, **extra_kw)
        res[0].backward()
        out.append((res, tq.grad, tc.grad))
        return out
    for (ra, gqa, gca), (rb, gqb, gcb) in zip(run((), {}), run(("KD_softmax",), dict(dkd_alpha=1.0, dkd_beta=8.0))):
        assert torch.equal(gqa, gqb) and torch.equal(gca, gcb)
        for a, b in zip(ra, rb):
            if rows == 2:
                assert torch.equal(a, b)
            else:
                assert abs(a.item() - b.item()) <= 1e-6 * max(1.0, abs(a.item()))


@pytest.mark.parametrize("C", [24, 130])
def test_all_pairs_forms_agree_on_the_hard_term(dev, C):
    """What every objective of the all-pairs row kernel shares -- lse = m + log(s1), hard = (lse - S[pos]) / Q, the arg-max
    count -- is the same bits whichever objective runs: the NLL loss (loss_scale 1) == the hard term of each kd_type.  Two rows,
    so that the atomic sum of the rows has one order; C below one lane stride and with a tail after two."""
    from simxns_amd import ops
    Q, H = 2, 64
    rs = np.random.RandomState(C)
    q, c, tq_, tc_ = _emb(rs, Q, H), _emb(rs, C, H), _emb(rs, Q, H), _emb(rs, C, H)
    pos = [0, C - 1]
    nll, nll_correct = ops.inbatch_nll_loss(_t(q, dev), _t(c, dev), pos, 1.0)
    for kd_type in BI_TYPES:
        _, hard, _, correct = ops.bi_kd_loss(_t(q, dev), _t(c, dev), _t(tq_, dev), _t(tc_, dev), pos, HP["T"], HP["ce_w"], HP["kd_w"],
                                             1.0, None, None, kd_type, HP["alpha"], HP["beta"])
        print("%s C%d: nll %s hard %s" % (kd_type, C, float(nll.item()).hex(), float(hard.item()).hex()))
        assert torch.equal(nll, hard), kd_type
        assert torch.equal(nll_correct, correct), kd_type


# ------------------------------------------------------------------------------------------ SIMX_DETERMINISTIC=1
def _det_worker(out_path):
    """Every new kernel path once, many rows (so that the atomic order would matter), bits of the results to ``out_path``."""
    from simxns_amd import _lib, ops
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(77)
    B, D, H, Q, C = 67, 16, 64, 67, 130
    q, c, z = _emb(rs, B, H), _emb(rs, B * D, H), _f32(rs.randn(B, D) * 2.0)
    q2, c2, tq_, tc_ = _emb(rs, Q, H), _emb(rs, C, H), _emb(rs, Q, H), _emb(rs, C, H)
    pos = [(7 * i) % C for i in range(Q)]
    rec = {"det": int(_lib.load().simx_deterministic())}

    def note(key, res, tq, tc):
        res[0].backward()
        torch.cuda.synchronize()
        rec[key] = [float(v.item()).hex() for v in res] + [hashlib.sha256(g.grad.cpu().numpy().tobytes()).hexdigest() for g in (tq, tc)]
    for kd_type in CROSS_TYPES[1:]:
        tq, tc = _t(q, dev, True), _t(c, dev, True)
        note("cross." + kd_type, ops.cross_kd_loss(tq, tc, _t(z, dev), 4.0, 0.1, 0.9, kd_type, 1.0, 8.0), tq, tc)
    for kd_type in BI_TYPES[1:]:
        tq, tc = _t(q2, dev, True), _t(c2, dev, True)
        note("bi." + kd_type, ops.bi_kd_loss(tq, tc, _t(tq_, dev), _t(tc_, dev), pos, 4.0, 0.1, 0.9, 2.0, (3, 40), (5, 100), kd_type, 1.0, 8.0), tq, tc)
    with open(out_path, "w") as f:
        json.dump(rec, f)


def _det_run(tmp_path, tag):
    out = str(tmp_path / ("%s.json" % tag))
    env = dict(os.environ)
    env["SIMX_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    code = "from test_kd_variants_gpu import _det_worker; _det_worker(%r)" % out
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out) as f:
        return json.load(f)


def test_kd_variants_deterministic_mode(tmp_path):
    """SIMX_DETERMINISTIC=1 (read once per process, hence the two fresh children): identical bits for every new kernel path."""
    a, b = _det_run(tmp_path, "a"), _det_run(tmp_path, "b")
    assert a["det"] == 1 and b["det"] == 1
    assert set(a) == {"det"} | {"cross." + k for k in CROSS_TYPES[1:]} | {"bi." + k for k in BI_TYPES[1:]}
    assert a == b


# ------------------------------------------------------------------------------------------ the distillation step
def _tiny_step(dev, **kw):
    """cross_encoder_distill_step on a two-layer student / teacher / frozen copy -> (loss, {student parameter: gradient})."""
    from oracle.weights import BertCfg, TINY, make_batch, make_bert_params
    from simxns_amd.engine import BertConfigLite
    from simxns_amd.ProD_KD.model.models import BiBertEncoder, HFBertEncoder, Reranker
    from simxns_amd.ProD_KD.run_progressive_distill_marco import cross_encoder_distill_step
    ocfg = BertCfg(**TINY)
    cfg = BertConfigLite(vocab_size=ocfg.vocab, hidden_size=ocfg.hidden, num_hidden_layers=ocfg.layers, num_attention_heads=ocfg.heads,
                         intermediate_size=ocfg.inter, max_position_embeddings=ocfg.max_pos, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0)

    def enc(seed):
        m = HFBertEncoder(cfg, compute_dtype="fp32")
        m.load_numpy_state(make_bert_params(ocfg, seed, std=0.08))
        return m

    def bi(sq, sc):
        m = BiBertEncoder.__new__(BiBertEncoder)
        torch.nn.Module.__init__(m)
        m.question_model, m.ctx_model = enc(sq), enc(sc)
        return m.to(dev)
    model, copy_, teacher = bi(1, 2), bi(3, 4), Reranker(enc(5), ocfg.hidden).to(dev)
    B, N = 3, 3
    t = lambda a: torch.from_numpy(a).to(dev)
    q_ids, q_mask, _ = make_batch(21, B, 16, ocfg.vocab, 9, 3, 4)
    c_ids, c_mask, _ = make_batch(22, B * (1 + N), 32, ocfg.vocab, 20, 6, 8)
    x_ids, x_mask, _ = make_batch(23, B * (1 + N), 48, ocfg.vocab, 30, 8, 12)
    args = dict(KD_type="KD_softmax", TEMPERATURE=4.0, CE_WEIGHT=0.1, KD_WEIGHT=0.9, LwF_WEIGHT=1.0, DKD_alpha=1.0, DKD_beta=8.0,
                open_LwF=False, gradient_accumulation_steps=1, max_grad_norm=2.0)
    args.update(kw)
    model.train()
    model.zero_grad()
    loss, _ = cross_encoder_distill_step(
        types.SimpleNamespace(**args), model, teacher,
        dict(query_ids=t(q_ids), attention_mask_q=t(q_mask), input_ids_a=t(c_ids), attention_mask_a=t(c_mask)),
        dict(input_ids=t(x_ids).view(B, 1 + N, -1), attention_mask=t(x_mask).view(B, 1 + N, -1)),
        student_copy=copy_ if args["open_LwF"] else None)
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def softmax_step(dev):
    return _tiny_step(dev)


@pytest.mark.parametrize("kw", [dict(KD_type="DKD"), dict(KD_type="KD_logit", open_LwF=True)], ids=["DKD", "KD_logit+LwF"])
def test_distill_step_with_kd_variant(dev, softmax_step, kw):
    _, base = softmax_step
    loss, grads = _tiny_step(dev, **kw)
    assert np.isfinite(loss)
    live = [k for k, g in base.items() if np.abs(g).max() > 0]
    assert len(live) > 30 and set(grads) == set(base)
    for k in live:
        assert np.isfinite(grads[k]).all() and np.abs(grads[k]).max() > 0, k
    pool = [k for k in grads if ".pooler." in k]
    assert len(pool) == 4
    for k in pool:
        assert np.abs(grads[k]).max() == 0.0, k
