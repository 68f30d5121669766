"""Float64 NumPy restatement of the LEAD slot objective and its four gradients (simx_lead_scores_fwd_bwd, include/simx.h).

TEST INFRASTRUCTURE only, the companion of tools/make_lead_golden.py: tests/test_lead_cpu.py holds it against the imported
reference's autograd (tests/golden/lead_losses.npz), so the closed forms the kernels implement are pinned without a GPU.
It is not a fallback of the package: simxns_amd never imports it.

Per slot, S = q ctx^T, Z = tq tctx^T, p = softmax(S), v = softmax(S/T), r = softmax(Z), u = softmax(Z/T):
  slot loss = a nll_s + b nll_t + w kl_ts + x kl_st
  dS = [a (p - e_pos) + w (p - u) + (x/T) v (h - sum_c v h)] / Q,  h = log v - log r
  dZ = [b (r - e_pos) + x (r - v) + (w/T) u (g - sum_c u g)] / Q,  g = log u - log p
A slot flagged ``reweight`` takes w = softmax_i(-nll_t,i / layer_temperature) over the flagged slots, a constant that the
reference rounds to float32 (torch.tensor of Python floats) before its softmax: ``f32_lambda`` does the same.
"""
import numpy as np


def _log_softmax(x):
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def _xlogy_diff(pr, la, lb):
    """sum_c pr (la - lb) per row with 0 log 0 = 0."""
    return np.where(pr > 0, pr * (la - lb), 0.0).sum(axis=1)


def lead_loss(q, ctx, tq, tctx, pos, slots, T, layer_temperature, loss_scale=1.0, local_q=None, local_ctx=None,
              f32_lambda=True):
    """q [n,Q,H], ctx [n,C,H], tq [n,Q,HT], tctx [n,C,HT]; slots: n x (a, b, w, x, reweight).
    -> dict(total, slot_losses [n,4], weights [n], dq, dctx, dtq, dtctx) with the gradients of the local rows only."""
    q, ctx, tq, tctx = (np.asarray(t, dtype=np.float64) for t in (q, ctx, tq, tctx))
    pos = np.asarray(pos, dtype=np.int64)
    n, Q, _ = q.shape
    C = ctx.shape[1]
    q_lo, q_n = local_q if local_q is not None else (0, Q)
    c_lo, c_n = local_ctx if local_ctx is not None else (0, C)
    rows = np.arange(Q)
    hot = np.zeros((Q, C))
    hot[rows, pos] = 1.0
    st = []
    losses = np.zeros((n, 4))
    for i in range(n):
        S, Z = q[i] @ ctx[i].T, tq[i] @ tctx[i].T
        lp, lv, lr, lu = _log_softmax(S), _log_softmax(S / T), _log_softmax(Z), _log_softmax(Z / T)
        u, v = np.exp(lu), np.exp(lv)
        kts, kst = _xlogy_diff(u, lu, lp), _xlogy_diff(v, lv, lr)
        losses[i] = (-lp[rows, pos].mean(), -lr[rows, pos].mean(), kts.sum() / Q, kst.sum() / Q)
        st.append((lp, lv, lr, lu, kts, kst))
    flagged = [i for i in range(n) if slots[i][4]]
    weights = np.array([s[2] for s in slots], dtype=np.float64)
    if flagged:
        e = np.array([-losses[i, 1] / layer_temperature for i in flagged])
        if f32_lambda:
            e = e.astype(np.float32)
        e = np.exp(e - e.max())
        weights[flagged] = (e / e.sum()).astype(np.float64)
    total = 0.0
    out = dict(dq=[], dctx=[], dtq=[], dtctx=[])
    for i in range(n):
        a, b, _, x, _ = slots[i]
        w = weights[i]
        total += a * losses[i, 0] + b * losses[i, 1] + w * losses[i, 2] + x * losses[i, 3]
        lp, lv, lr, lu, kts, kst = st[i]
        p, v, r, u = np.exp(lp), np.exp(lv), np.exp(lr), np.exp(lu)
        dS = (a * (p - hot) + w * (p - u) + (x / T) * v * ((lv - lr) - kst[:, None])) * (loss_scale / Q)
        dZ = (b * (r - hot) + x * (r - v) + (w / T) * u * ((lu - lp) - kts[:, None])) * (loss_scale / Q)
        out["dq"].append((dS @ ctx[i])[q_lo:q_lo + q_n])
        out["dctx"].append((dS.T @ q[i])[c_lo:c_lo + c_n])
        out["dtq"].append((dZ @ tctx[i])[q_lo:q_lo + q_n])
        out["dtctx"].append((dZ.T @ tq[i])[c_lo:c_lo + c_n])
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(total=total * loss_scale, slot_losses=losses, weights=weights)
    return out


def slots_for(n_layers, reweight, train_de, para_db, para_de, para_dis, para_layer):
    """The slot weights of distill_loss for distill_de + distill_db + distill_de_db_layer_score: n_layers layer slots
    (a = b = x = 0, w = lambda or para_layer) followed by the final slot of the pooled embeddings."""
    layer = [(0.0, 0.0, 0.0 if reweight else para_layer, 0.0, 1 if reweight else 0)] * n_layers
    final = (para_db, para_de if train_de else 0.0, para_dis, para_dis if train_de else 0.0, 0)
    return layer + [final]
