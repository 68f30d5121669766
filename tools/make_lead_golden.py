"""Write the LEAD fixtures from the IMPORTED REFERENCE (LEAD/util.py: distill_loss, select_layer) in float64 with autograd.

TEST INFRASTRUCTURE, in the style of tools/make_kd_golden.py; it needs a checkout of the reference project (not needed to
build, test or run the package), only the fixtures travel.  Run:  python -m tools.make_lead_golden [--reference DIR]

LEAD/util.py does not import under a current transformers: its sibling models.py imports the vendored modeling_bert.py, which
fails.  The loss functions use neither models nor dataset, so both are replaced in sys.modules by empty stand-ins first.

tests/golden/lead_losses.npz -- distill_loss for distill_de + distill_db + distill_de_db_layer_score.  Slot order: the layer
  slots, then the final slot of the pooled embeddings.  Per case "<case>.<what>": q [n,Q,H], ctx [n,C,H], tq [n,Q,HT],
  tctx [n,C,HT] (float32), pos, slots [n,5] = (a, b, w, x, reweight), T, LT, loss, weights [n] (the w the reference applied),
  slot_losses [n,4] = (nll_s, nll_t, kl_ts, kl_st), every loss_dict entry as dict.<key>, and dq, dctx, dtq, dtctx.
    i    Q=5, neg=3 (C=20), H=32, HT=48, three layer slots from 6 / 12 layers, T=2, layer_temperature=0.5, reweight, train_de
    ii   the same without reweight, distill_para_de_db_layer_score = 0.6
    iii  i with train_de off (autograd still reaches the teacher through the KL target: stored, the caller decides)
    iv   Q=10, neg=12 (C=130), T=1, layer_temperature=10, one layer slot (lambda = 1)
    v.r0, v.r1  case i as the two ranks of a gathered W = 2 batch see it: rank 0 owns queries 0-2, rank 1 queries 3-4 (with
         their passages); only the own rows are leaves, the rest constants (gather_tensor keeps the local tensor in its slot)
tests/golden/lead_step_tiny.npz -- one whole step (two forwards with all hidden states, distill_loss, backward) on the tiny
  geometry: loss, loss_dict, embeddings, the tapped [CLS] rows, gradient norms and slices of both towers (gen_step).
tests/golden/lead_select_layer.json -- select_layer after random.seed(888), three calls, for each selection mode x
  {ms, other} train-file name x {base, large} x add_linear.
"""
import argparse
import io
import itertools
import json
import os
import random
import sys
import types
import warnings
from contextlib import redirect_stdout

import numpy as np
import torch

from oracle.make_golden import REF, _load
from tools.lead_ref import slots_for

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
PARA_DB, PARA_DE, PARA_DIS, PARA_LAYER = 0.7, 1.3, 0.45, 0.6       # distinct and non-unit: no two can be swapped unnoticed


def load_reference_util(ref):
    for name, attrs in (("models", ("BiBertEncoder", "HFBertEncoder", "Reranker")), ("dataset", ("TraditionDataset",))):
        stand_in = types.ModuleType(name)
        for a in attrs:
            setattr(stand_in, a, None)
        sys.modules[name] = stand_in
    try:
        return _load("ref_lead_util", os.path.join(ref, "LEAD/util.py"))
    finally:
        for name in ("models", "dataset"):
            del sys.modules[name]


def _args(T, LT, reweight, train_de):
    return types.SimpleNamespace(
        device="cpu", local_rank=-1, rank=0, distill_db=True, distill_de=True, distill_col=False, distill_ce=False, train_de=train_de,
        train_col=False, train_ce=False, temperature=T, layer_temperature=LT, layer_score_reweight=reweight,
        distill_de_db_layer_score=True, distill_col_db_layer_score=False, distill_ce_db_layer_score=False,
        distill_de_db_attention=False, distill_col_db_attention=False, distill_ce_db_attention=False,
        distill_para_db=PARA_DB, distill_para_de=PARA_DE, distill_para_de_db_dis=PARA_DIS, distill_para_de_db_layer_score=PARA_LAYER)


def _inputs(rs, Q, neg, H, HT, n_layer, align_s, align_t):
    """n_layer layer slots + the final slot; every other query finds its positive, by a per-slot margin."""
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    C = Q * (1 + neg)
    pos = np.arange(Q) * (1 + neg)
    n = n_layer + 1
    x = dict(q=f32(rs.randn(n, Q, H) * 0.6), ctx=f32(rs.randn(n, C, H) * 0.6), tq=f32(rs.randn(n, Q, HT) * 0.5),
             tctx=f32(rs.randn(n, C, HT) * 0.5))
    for i in range(n):
        x["ctx"][i][pos[0::2]] = f32(x["ctx"][i][pos[0::2]] + align_s[i] * x["q"][i][0::2])
        x["tctx"][i][pos[0::2]] = f32(x["tctx"][i][pos[0::2]] + align_t[i] * x["tq"][i][0::2])
        for a, b, who in ((x["q"][i], x["ctx"][i], "student"), (x["tq"][i], x["tctx"][i], "teacher")):
            ok = int(((a @ b.T).argmax(1) == pos).sum())
            assert 0 < ok < Q, "slot %d (%s) needs a correctly and a wrongly ranked query (%d of %d correct)" % (i, who, ok, Q)
    return x, pos


def _run(U, args, x, pos, sel_s, sel_t, L_s, L_t, own_q=None, own_c=None):
    """distill_loss on the slot vectors placed at the selected layers of [rows, layers, 1, width] hidden-state tensors; the
    rows [lo, lo+n) of own_q / own_c are leaves, the others constants.  -> (loss, loss_dict, grads [n, rows_local, width] x 4)."""
    n_layer = len(sel_s)
    Q, C = x["q"].shape[1], x["ctx"].shape[1]
    q_lo, q_n = own_q if own_q is not None else (0, Q)
    c_lo, c_n = own_c if own_c is not None else (0, C)
    leaves = {}

    def gathered(key, i, lo, cnt):
        a = x[key][i]
        leaf = torch.tensor(a[lo:lo + cnt], dtype=torch.float64, requires_grad=True)
        leaves[(key, i)] = leaf
        parts = [torch.tensor(a[:lo], dtype=torch.float64), leaf, torch.tensor(a[lo + cnt:], dtype=torch.float64)]
        return torch.cat(parts, 0)

    def hidden(key, sel, layers, lo, cnt):
        rows, width = x[key].shape[1], x[key].shape[2]
        per_layer = [torch.zeros(rows, width, dtype=torch.float64) for _ in range(layers)]
        for i, l in enumerate(sel):
            per_layer[l] = gathered(key, i, lo, cnt)
        return torch.stack(per_layer, 1).unsqueeze(2)
    q_h, c_h = hidden("q", sel_s, L_s, q_lo, q_n), hidden("ctx", sel_s, L_s, c_lo, c_n)
    tq_h, tc_h = hidden("tq", sel_t, L_t, q_lo, q_n), hidden("tctx", sel_t, L_t, c_lo, c_n)
    fin = n_layer
    batch = {"de_ctx_start_end": torch.zeros(Q, C // Q, 2, dtype=torch.long)}
    loss, d = U.distill_loss(args, None, gathered("tq", fin, q_lo, q_n), gathered("q", fin, q_lo, q_n), None,
                             gathered("tctx", fin, c_lo, c_n), gathered("ctx", fin, c_lo, c_n), None, sel_s, sel_t, None,
                             tq_h, tc_h, q_h, c_h, None, None, None, None, None, batch)
    loss.backward()
    g = {k: np.stack([leaves[(k, i)].grad.numpy().copy() if leaves[(k, i)].grad is not None else np.zeros_like(leaves[(k, i)].detach().numpy())
                      for i in range(n_layer + 1)]) for k in ("q", "ctx", "tq", "tctx")}
    return loss, d, g


def _put(out, case, x, pos, slots, T, LT, loss, d, g, weights, slot_losses, store_inputs=True):
    vals = dict(loss=np.float64(loss.item()), dq=g["q"], dctx=g["ctx"], dtq=g["tq"], dtctx=g["tctx"], weights=weights,
                slot_losses=slot_losses, slots=np.asarray(slots, dtype=np.float64), T=np.float64(T), LT=np.float64(LT))
    for k, v in d.items():
        vals["dict." + k] = np.float64(float(v))
    for k, v in vals.items():
        assert np.isfinite(v).all(), "%s.%s is not finite" % (case, k)
        out["%s.%s" % (case, k)] = v
    if store_inputs:
        out.update({"%s.%s" % (case, k): v.astype(np.float32) for k, v in x.items()})
        out["%s.pos" % case] = pos.astype(np.int64)
    print(" %-6s loss %.12f weights %s |dq| %.3e |dtq| %.3e" % (case, vals["loss"], np.array2string(weights, precision=4),
                                                                np.abs(g["q"]).max(), np.abs(g["tq"]).max()))


def _terms(d, n_layer, reweight, train_de, x, pos, T):
    """slot_losses [n,4] and the applied weights, read back from the reference's loss_dict where it reports them and from its
    own formulas (torch, float64) where it does not (the layer slots' teacher NLL, the student-side layer terms)."""
    import torch.nn.functional as F
    n = n_layer + 1
    sl = np.zeros((n, 4))
    tgt = torch.tensor(pos)
    for i in range(n):
        S = torch.tensor(x["q"][i] @ x["ctx"][i].T)
        Z = torch.tensor(x["tq"][i] @ x["tctx"][i].T)
        ls, lz = F.log_softmax(S, -1), F.log_softmax(Z, -1)
        sl[i] = (F.nll_loss(ls, tgt).item(), F.nll_loss(lz, tgt).item(),
                 F.kl_div(ls, F.softmax(Z / T, -1), reduction="batchmean").item(),
                 F.kl_div(lz, F.softmax(S / T, -1), reduction="batchmean").item())
    for i in range(n_layer):
        assert abs(sl[i, 2] - float(d["loss_score_layer_dis_%d" % i])) < 1e-12
    assert abs(sl[n_layer, 0] - float(d["loss_db"])) < 1e-12 and abs(sl[n_layer, 2] - float(d["loss_de_db_dis"])) < 1e-12
    assert abs(sl[n_layer, 3] - float(d["loss_db_de_dis"])) < 1e-12
    if train_de:
        assert abs(sl[n_layer, 1] - float(d["loss_dual"])) < 1e-12
    return sl


def gen_losses(U):
    rs = np.random.RandomState(31)
    out = {}
    H, HT, T, LT = 32, 48, 2.0, 0.5
    sel_s, sel_t = [1, 3, 4], [2, 7, 11]
    x, pos = _inputs(rs, 5, 3, H, HT, 3, align_s=(0.6, 0.9, 1.2, 0.8), align_t=(0.9, 1.8, 3.2, 1.0))
    for case, reweight, train_de in (("i", True, True), ("ii", False, True), ("iii", True, False)):
        a = _args(T, LT, reweight, train_de)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss, d, g = _run(U, a, x, pos, sel_s, sel_t, 6, 12)
        sl = _terms(d, 3, reweight, train_de, x, pos, T)
        slots = slots_for(3, reweight, train_de, PARA_DB, PARA_DE, PARA_DIS, PARA_LAYER)
        w = np.array([s[2] for s in slots])
        if reweight:
            lam = torch.softmax(torch.tensor([-v / LT for v in sl[:3, 1]]), 0).double().numpy()    # float32, as the reference forms it
            w[:3] = lam
            assert abs(float(d["loss_de_db_layer_dis"]) - float((lam * sl[:3, 2]).sum())) < 1e-12
            if case == "i":
                assert lam.max() / lam.min() >= 3.0, "lambda spread %.2f < 3: a wrong lambda could hide in the tolerance" % (lam.max() / lam.min())
        _put(out, case, x, pos, slots, T, LT, loss, d, g, w, sl)
        if case == "i":
            base = (loss, sl, w, slots)
    # v: the same batch gathered from two ranks
    for r, (own_q, own_c) in enumerate((((0, 3), (0, 12)), ((3, 2), (12, 8)))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss, d, g = _run(U, _args(T, LT, True, True), x, pos, sel_s, sel_t, 6, 12, own_q, own_c)
        assert abs(loss.item() - base[0].item()) < 1e-12
        _put(out, "v.r%d" % r, x, pos, base[3], T, LT, loss, d, g, base[2], base[1], store_inputs=False)
        out["v.r%d.local_q" % r], out["v.r%d.local_ctx" % r] = np.asarray(own_q, dtype=np.int64), np.asarray(own_c, dtype=np.int64)
    # iv: the recipe's temperatures, three 64-lane passes with a 2-lane tail, one layer slot
    T4, LT4 = 1.0, 10.0
    x4, pos4 = _inputs(rs, 10, 12, H, HT, 1, align_s=(1.2, 1.0), align_t=(1.5, 1.3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, d, g = _run(U, _args(T4, LT4, True, True), x4, pos4, [2], [5], 6, 12)
    sl = _terms(d, 1, True, True, x4, pos4, T4)
    slots = slots_for(1, True, True, PARA_DB, PARA_DE, PARA_DIS, PARA_LAYER)
    w = np.array([1.0, PARA_DIS])
    _put(out, "iv", x4, pos4, slots, T4, LT4, loss, d, g, w, sl)
    path = os.path.join(GOLDEN, "lead_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


STEP = dict(B=4, neg=3, q_len=32, p_len=128, teacher_layers=4, student_layers=2, sel_db=[0, 1], sel_teacher=[1, 3], T=2.0, LT=0.5,
            seeds=(4101, 4102), std=0.08)


def gen_step(U):
    """tests/golden/lead_step_tiny.npz: one whole LEAD step (run_LEAD.py:156-227) in float64 on the tiny geometry of
    oracle/make_golden.py -- a 4-layer teacher and a 2-layer student, each ONE shared tower for queries and passages, B = 4,
    3 negatives, q32 / p128, dropout off, student layers [0, 1] paired with teacher layers [1, 3], the flags of case i.

    The encoders are transformers.BertModel(output_hidden_states=True) read as hidden_states[1:] and last_hidden_state[:, 0]:
    that is what the reference's vendored HFBertEncoder returns (LEAD/modeling_bert.py:617-626 collects the output of every
    encoder layer, without the embedding output; LEAD/models.py takes row 0 of the last one as pooled_output).  The vendored
    class itself is not imported: modeling_bert.py is a copy of a transformers 2.x file and fails to import against the
    installed transformers, whose BertModel computes the same function."""
    from transformers import BertConfig, BertModel
    from oracle.weights import BertCfg, TINY, make_batch, make_bert_params
    S = STEP
    tcfg, scfg = BertCfg(**dict(TINY, layers=S["teacher_layers"])), BertCfg(**dict(TINY, layers=S["student_layers"]))

    def tower(cfg, seed):
        hf = BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                        intermediate_size=cfg.inter, max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab,
                        layer_norm_eps=cfg.eps, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        output_hidden_states=True, attn_implementation="eager")
        m = BertModel(hf)
        P = make_bert_params(cfg, seed, std=S["std"])
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=False)
        assert not [k for k in missing if "position_ids" not in k] and not unexpected, (missing, unexpected)
        return m.double().train()

    def encode(m, ids, mask):
        out = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))
        hidden = torch.cat([h.unsqueeze(0) for h in out.hidden_states[1:]], 0).permute([1, 0, 2, 3])
        return out.last_hidden_state[:, 0, :], hidden
    model_de, model_db = tower(tcfg, S["seeds"][0]), tower(scfg, S["seeds"][1])
    B, C = S["B"], S["B"] * (1 + S["neg"])
    q_ids, q_mask, _ = make_batch(S["seeds"][0] + 100, B, S["q_len"], tcfg.vocab, 9, 3, 4)
    d_ids, d_mask, _ = make_batch(S["seeds"][1] + 100, C, S["p_len"], tcfg.vocab, 80, 25, 16)
    args = _args(S["T"], S["LT"], True, True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q_db, qh_db = encode(model_db, q_ids, q_mask)
        d_db, dh_db = encode(model_db, d_ids, d_mask)
        q_de, qh_de = encode(model_de, q_ids, q_mask)
        d_de, dh_de = encode(model_de, d_ids, d_mask)
        batch = {"de_ctx_start_end": torch.zeros(B, 1 + S["neg"], 2, dtype=torch.long)}
        loss, d = U.distill_loss(args, None, q_de, q_db, None, d_de, d_db, None, S["sel_db"], S["sel_teacher"], None, qh_de, dh_de,
                                 qh_db, dh_db, None, None, None, None, None, batch)
        loss.backward()
    npy = lambda t: t.detach().numpy()
    taps = lambda h, sel: np.stack([npy(h[:, l, 0, :]) for l in sel])
    out = dict(q_ids=q_ids, q_mask=q_mask, d_ids=d_ids, d_mask=d_mask, seeds=np.asarray(S["seeds"]), std=np.float64(S["std"]),
               layers=np.asarray([S["teacher_layers"], S["student_layers"]]), sel_db=np.asarray(S["sel_db"]),
               sel_teacher=np.asarray(S["sel_teacher"]), T=np.float64(S["T"]), LT=np.float64(S["LT"]),
               paras=np.asarray([PARA_DB, PARA_DE, PARA_DIS, PARA_LAYER]), loss=np.float64(loss.item()),
               q_db=npy(q_db), d_db=npy(d_db), q_de=npy(q_de), d_de=npy(d_de), q_taps_db=taps(qh_db, S["sel_db"]),
               d_taps_db=taps(dh_db, S["sel_db"]), q_taps_de=taps(qh_de, S["sel_teacher"]), d_taps_de=taps(dh_de, S["sel_teacher"]))
    for k, v in d.items():
        out["dict." + k] = np.float64(float(v))
    for role, m in (("de", model_de), ("db", model_db)):
        Gr = {k: p.grad.detach().numpy().astype(np.float64) for k, p in m.named_parameters() if p.grad is not None}
        names = sorted(Gr)
        out[role + ".grad_names"] = np.asarray(names)
        out[role + ".grad_norms"] = np.asarray([np.sqrt((Gr[k] ** 2).sum()) for k in names])
        for k in names:
            out["%s.gslice.%s" % (role, k)] = Gr[k][:8, :64] if Gr[k].ndim == 2 else Gr[k]
    for k, v in out.items():
        assert np.asarray(v).dtype.kind in "US" or np.isfinite(v).all(), k
    lam = torch.softmax(torch.tensor([-float(torch.nn.functional.nll_loss(torch.log_softmax(torch.from_numpy(
        out["q_taps_de"][i] @ out["d_taps_de"][i].T), -1), torch.arange(0, C, 1 + S["neg"]))) / S["LT"] for i in range(2)]), 0)
    print(" step   loss %.12f lambda %s |g_de| %.3e |g_db| %.3e" % (out["loss"], lam.numpy(), out["de.grad_norms"].max(), out["db.grad_norms"].max()))
    path = os.path.join(GOLDEN, "lead_step_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def gen_select_layer(U):
    out = []
    modes = ("layer_selection_random", "layer_selection_last", "layer_selection_skip")
    for mode, train_file, name, add_linear in itertools.product(modes, ("data/ms_train.json", "data/nq-train.json"),
                                                                ("bert-base-uncased", "bert-large-uncased"), (False, True)):
        a = types.SimpleNamespace(pretrained_model_name=name, train_file=train_file, add_linear=add_linear, disitll_layer_num=5,
                                  **{m: m == mode for m in modes})
        random.seed(888)
        with redirect_stdout(io.StringIO()):
            picks = [U.select_layer(a) for _ in range(3)]
        out.append(dict(mode=mode, train_file=train_file, pretrained_model_name=name, add_linear=add_linear, disitll_layer_num=5,
                        seed=888, picks=[[list(p[0]), list(p[1])] for p in picks]))
    path = os.path.join(GOLDEN, "lead_select_layer.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote %s (%d cases)" % (path, len(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF, help="checkout of the reference project")
    ref = ap.parse_args().reference
    U = load_reference_util(ref)
    gen_losses(U)
    gen_step(U)
    gen_select_layer(U)


if __name__ == "__main__":
    main()
