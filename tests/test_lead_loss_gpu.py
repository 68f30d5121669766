"""GPU: the LEAD slot loss (simx_lead_scores_fwd_bwd, ops.lead_layer_score_loss) against the imported reference's float64
autograd (tests/golden/lead_losses.npz), the existing KD_softmax unit, and itself (run-to-run bits, rejected arguments)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_lead_cpu import CASES, case_inputs

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


def _close(got, ref, tol=3e-5, what=""):
    """The rule of tests/test_kd_variants_gpu.py: 3e-5 of max(1, |ref|max)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max()
    lim = tol * max(1.0, np.abs(ref).max())
    print("%s: err %.3e (bound %.3e)" % (what, err, lim))
    assert err <= lim, "%s: err %.3e > %.3e" % (what, err, lim)


def _t(a, dev, req=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).requires_grad_(req)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "lead_losses.npz"))


def _raw(dev, q, ctx, tq, tctx, pos, slots, T, LT, lq=None, lc=None, teacher_grad=1, loss_scale=1.0, ws_short=0, **over):
    """One direct call of the C ABI -> (rc, dict of output tensors); ``over`` replaces scalar arguments by name."""
    from simxns_amd import _lib as L
    lib = L.load()
    q, ctx, tq, tctx = (_t(a, dev) for a in (q, ctx, tq, tctx))
    n, Q, H = q.shape
    Cn, HT = ctx.shape[1], tq.shape[2]
    q_lo, q_n = lq if lq is not None else (0, Q)
    c_lo, c_n = lc if lc is not None else (0, Cn)
    a = dict(n=n, Q=Q, C=Cn, H=H, HT=HT, T=T, LT=LT, q_lo=q_lo, q_n=q_n, c_lo=c_lo, c_n=c_n)
    a.update(over)
    f = lambda *sh: torch.full(sh, SENTINEL, dtype=torch.float32, device=dev)
    o = dict(scores=f(n, Q, Cn), tscores=f(n, Q, Cn), slot_losses=f(n, 4), weights=f(n), total=f(1), dq=f(n, max(q_n, 1), H),
             dctx=f(n, max(c_n, 1), H), dtq=f(n, max(q_n, 1), HT), dtctx=f(n, max(c_n, 1), HT))
    wsb = int(lib.simx_lead_scores_workspace_bytes(n, Q, Cn, H, HT, q_n, c_n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    arr = (L.LeadSlot * n)(*[L.LeadSlot(*s) for s in slots])
    post = torch.as_tensor(pos, dtype=torch.int32, device=dev)
    null = over.get("null")
    p = lambda k, t: None if null == k else L.ptr(t)
    rc = lib.simx_lead_scores_fwd_bwd(L.stream_ptr(), a["n"], a["Q"], a["C"], a["H"], a["HT"], p("q", q), L.ptr(ctx), L.ptr(tq), L.ptr(tctx),
                                      L.ptr(post), a["T"], a["LT"], arr, teacher_grad, loss_scale, a["q_lo"], a["q_n"], a["c_lo"], a["c_n"],
                                      L.ptr(o["scores"]), L.ptr(o["tscores"]), L.ptr(o["slot_losses"]), p("weights", o["weights"]),
                                      L.ptr(o["total"]), L.ptr(o["dq"]), L.ptr(o["dctx"]), p("dtq", o["dtq"]), L.ptr(o["dtctx"]),
                                      p("ws", ws), wsb - ws_short)
    torch.cuda.synchronize()
    return rc, o


def _check_losses(G, case, total, slot_losses, weights, scale=1.0):
    _close(total, scale * float(G[case + ".loss"]), what=case + " total")
    _close(slot_losses, G[case + ".slot_losses"], what=case + " slot_losses")
    _close(weights, G[case + ".weights"], what=case + " weights")


@pytest.mark.parametrize("case", CASES)
def test_lead_loss_golden_ops(dev, G, case):
    from simxns_amd import ops
    q, ctx, tq, tctx, pos, slots, T, LT, lq, lc = case_inputs(G, case)
    ts = [_t(a, dev, True) for a in (q, ctx, tq, tctx)]
    total, sl, w = ops.lead_layer_score_loss(*ts, pos, slots, T, LT, teacher_grad=True, local_q=lq, local_ctx=lc)
    assert not sl.requires_grad and not w.requires_grad
    total.backward()
    _check_losses(G, case, total.item(), sl.cpu().numpy(), w.cpu().numpy())
    for t, k, loc in zip(ts, ("dq", "dctx", "dtq", "dtctx"), (lq, lc, lq, lc)):
        g = t.grad.cpu().numpy()
        lo, cnt = loc if loc is not None else (0, g.shape[1])
        _close(g[:, lo:lo + cnt], G["%s.%s" % (case, k)], what="%s %s" % (case, k))
        outside = np.delete(g, np.s_[lo:lo + cnt], axis=1)
        assert not outside.any(), "%s %s: gradient outside the local slot" % (case, k)


@pytest.mark.parametrize("case", CASES)
def test_lead_loss_golden_c_abi(dev, G, case):
    """The raw entry with loss_scale = 2: total and all four gradients scale, the slot losses and weights do not."""
    q, ctx, tq, tctx, pos, slots, T, LT, lq, lc = case_inputs(G, case)
    rc, o = _raw(dev, q, ctx, tq, tctx, pos, slots, T, LT, lq, lc, teacher_grad=1, loss_scale=2.0)
    assert rc == 0
    _check_losses(G, case, o["total"].item(), o["slot_losses"].cpu().numpy(), o["weights"].cpu().numpy(), scale=2.0)
    for k in ("dq", "dctx", "dtq", "dtctx"):
        _close(o[k].cpu().numpy(), 2.0 * G["%s.%s" % (case, k)], what="%s %s" % (case, k))


@pytest.mark.parametrize("case", ["iii", "v.r1"])
def test_teacher_buffers_untouched_without_teacher_grad(dev, G, case):
    q, ctx, tq, tctx, pos, slots, T, LT, lq, lc = case_inputs(G, case)
    rc, o = _raw(dev, q, ctx, tq, tctx, pos, slots, T, LT, lq, lc, teacher_grad=0)
    assert rc == 0
    assert bool((o["dtq"] == SENTINEL).all()) and bool((o["dtctx"] == SENTINEL).all())
    _check_losses(G, case, o["total"].item(), o["slot_losses"].cpu().numpy(), o["weights"].cpu().numpy())
    _close(o["dq"].cpu().numpy(), G[case + ".dq"], what=case + " dq")
    _close(o["dctx"].cpu().numpy(), G[case + ".dctx"], what=case + " dctx")
    ops_q = [_t(a, dev, r) for a, r in zip((q, ctx, tq, tctx), (True, True, True, True))]
    from simxns_amd import ops
    total, _, _ = ops.lead_layer_score_loss(*ops_q, pos, slots, T, LT, teacher_grad=False, local_q=lq, local_ctx=lc)
    total.backward()
    assert ops_q[2].grad is None and ops_q[3].grad is None and ops_q[0].grad is not None


@pytest.mark.parametrize("case", ["i", "iv"])
def test_single_slot_equals_kd_softmax_unit(dev, G, case):
    """n = 1 without reweight, b = x = 0, T = 1: a nll_s + w kl_ts is ce_w hard + kd_w T^2 soft of simx_scores_kd_type_fwd_bwd
    (SIMX_KD_SOFTMAX) on the same inputs -- loss, hard, soft and both gradients under the same rule."""
    from simxns_amd import ops
    q, ctx, tq, tctx, pos, _, _, _, _, _ = case_inputs(G, case)
    a, w = 0.7, 0.45
    last = slice(q.shape[0] - 1, q.shape[0])
    rc, o = _raw(dev, q[last], ctx[last], tq[last], tctx[last], pos, [(a, 0.0, w, 0.0, 0)], 1.0, 1.0, teacher_grad=0)
    assert rc == 0
    sq, sc = _t(q[-1], dev, True), _t(ctx[-1], dev, True)
    loss, hard, soft, _ = ops.bi_kd_loss(sq, sc, _t(tq[-1], dev), _t(tctx[-1], dev), pos, temperature=1.0, ce_weight=a, kd_weight=w)
    loss.backward()
    _close(o["total"].item(), loss.item(), what="total")
    _close(o["slot_losses"][0, 0].item(), hard.item(), what="hard")
    _close(o["slot_losses"][0, 2].item(), soft.item(), what="soft")
    _close(o["dq"][0].cpu().numpy(), sq.grad.cpu().numpy(), what="dq")
    _close(o["dctx"][0].cpu().numpy(), sc.grad.cpu().numpy(), what="dctx")
    assert o["weights"][0].item() == float(np.float32(w))


def test_two_runs_are_bit_identical(dev):
    """Many rows and five slots, SIMX_DETERMINISTIC unset: the per-slot sums are ordered reductions, so every output repeats."""
    assert os.environ.get("SIMX_DETERMINISTIC", "0") in ("", "0")
    rs = np.random.RandomState(5)
    n, Q, neg, H, HT = 5, 203, 2, 64, 40
    Cn = Q * (1 + neg)
    x = [rs.randn(n, Q, H) * 0.4, rs.randn(n, Cn, H) * 0.4, rs.randn(n, Q, HT) * 0.4, rs.randn(n, Cn, HT) * 0.4]
    pos = [i * (1 + neg) for i in range(Q)]
    slots = [(0.0, 0.0, 0.0, 0.0, 1)] * 4 + [(0.7, 1.3, 0.45, 0.45, 0)]
    runs = [_raw(dev, *x, pos, slots, 2.0, 0.5) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    assert abs(runs[0][1]["weights"][:4].sum().item() - 1.0) < 1e-5
    for k in ("total", "slot_losses", "weights", "dq", "dctx", "dtq", "dtctx"):
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("over,code", [
    (dict(n=0), -1), (dict(n=33), -1), (dict(T=0.0), -1), (dict(T=-1.0), -1), (dict(LT=0.0), -1), (dict(q_lo=4, q_n=2), -1),
    (dict(c_lo=-1), -1), (dict(c_n=21), -1), (dict(null="q"), -1), (dict(null="weights"), -1), (dict(null="dtq"), -1),
    (dict(null="ws"), -3), (dict(ws_short=1), -3)])
def test_rejected_arguments_launch_nothing(dev, G, over, code):
    """SIMX_ERR_BAD_SHAPE (-1) / SIMX_ERR_WORKSPACE (-3), and every output buffer still holds its sentinel."""
    from simxns_amd import _lib as L
    q, ctx, tq, tctx, pos, slots, T, LT, _, _ = case_inputs(G, "i")
    over = dict(over)
    ws_short, T, LT = over.pop("ws_short", 0), over.pop("T", T), over.pop("LT", LT)
    rc, o = _raw(dev, q, ctx, tq, tctx, pos, slots, T, LT, ws_short=ws_short, **over)
    assert rc == code, L.load().simx_last_error()
    for k, t in o.items():
        assert bool((t == SENTINEL).all()), k


def test_layer_temperature_only_matters_with_a_reweight_slot(dev, G):
    q, ctx, tq, tctx, pos, slots, T, _, _, _ = case_inputs(G, "ii")
    rc, o = _raw(dev, q, ctx, tq, tctx, pos, slots, T, 0.0)
    assert rc == 0
    _check_losses(G, "ii", o["total"].item(), o["slot_losses"].cpu().numpy(), o["weights"].cpu().numpy())


def test_wrapper_validates_before_the_device(dev):
    from simxns_amd import ops
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError):
        ops.lead_layer_score_loss(z(2, 3, 8), z(2, 6, 8), z(2, 3, 8), z(2, 6, 8), [0, 2, 4], [(1, 0, 1, 0, 0)], 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.lead_layer_score_loss(z(1, 3, 8), z(1, 6, 8), z(1, 4, 8), z(1, 6, 8), [0, 2, 4], [(1, 0, 1, 0, 0)], 1.0, 1.0)
