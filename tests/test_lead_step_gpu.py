"""GPU: one whole LEAD step (simxns_amd.LEAD.run_LEAD.lead_distill_step: two tapped forwards through shared towers, the slot
loss, backward into both towers) on the fp32 engine against the imported reference's float64 step
(tests/golden/lead_step_tiny.npz, tools/make_lead_golden.py::gen_step)."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _models(G, dev, dtype="fp32"):
    from simxns_amd.engine import BertConfigLite
    from simxns_amd.LEAD.models import BiBertEncoder
    from simxns_amd.model.models import HFBertEncoder
    from simxns_amd.utils import synth
    out = []
    for layers, seed in zip((int(v) for v in G["layers"]), (int(s) for s in G["seeds"])):
        cfg = BertConfigLite(vocab_size=1000, hidden_size=64, num_hidden_layers=layers, num_attention_heads=4, intermediate_size=128,
                             max_position_embeddings=192, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        enc = HFBertEncoder(cfg, compute_dtype=dtype)
        enc.load_numpy_state(synth.fill_bert_state_dict([(k, tuple(p.shape)) for k, p in enc.named_parameters()], seed, std=float(G["std"])))
        m = BiBertEncoder.__new__(BiBertEncoder)
        torch.nn.Module.__init__(m)
        m.question_model = m.ctx_model = enc                   # share_weight
        out.append(m.to(dev))
    return out                                                 # teacher (de), student (db)


def _args(G, **kw):
    db, de, dis, layer = (float(v) for v in G["paras"])
    a = dict(distill_de=True, distill_db=True, train_de=True, train_db=True, distill_de_db_layer_score=True, layer_score_reweight=True,
             temperature=float(G["T"]), layer_temperature=float(G["LT"]), distill_para_db=db, distill_para_de=de,
             distill_para_de_db_dis=dis, distill_para_de_db_layer_score=layer, gradient_accumulation_steps=1)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _grads(m):
    return {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.question_model.named_parameters() if p.grad is not None}


def test_lead_step_fp32_vs_reference_golden(dev, golden_dir):
    from simxns_amd.LEAD.run_LEAD import lead_distill_step
    G = np.load(os.path.join(golden_dir, "lead_step_tiny.npz"))
    model_de, model_db = _models(G, dev)
    batch = [torch.from_numpy(G[k]) for k in ("q_ids", "q_mask", "d_ids", "d_mask")]
    sel_db, sel_de = [int(v) for v in G["sel_db"]], [int(v) for v in G["sel_teacher"]]
    model_de.zero_grad(); model_db.zero_grad()
    loss, d = lead_distill_step(_args(G), model_de, model_db, batch, sel_db, sel_de)
    torch.cuda.synchronize()
    print("loss %.6f vs %.6f" % (loss.item(), float(G["loss"])))
    assert abs(loss.item() - float(G["loss"])) <= 1e-3
    keys = [k[len("dict."):] for k in G.files if k.startswith("dict.")]
    assert sorted(d) == sorted(keys)
    for k in keys:
        assert abs(float(d[k]) - float(G["dict." + k])) <= 1e-3, k
    # the pieces: embeddings and tapped [CLS] rows of both towers
    dev_batch = [t.to(dev) for t in batch]
    with torch.no_grad():
        for m, role, sel in ((model_de, "de", sel_de), (model_db, "db", sel_db)):
            m.eval()
            q, c, qt, ct, _ = m(*dev_batch, layers=sel)
            for got, key in ((q, "q_" + role), (c, "d_" + role), (qt, "q_taps_" + role), (ct, "d_taps_" + role)):
                err = np.abs(got.cpu().numpy() - G[key]).max()
                assert err <= 1e-3, "%s: %.3e" % (key, err)
    # gradients of both towers, by the rule of the PROD step test
    for m, role in ((model_de, "de"), (model_db, "db")):
        grads = _grads(m)
        names, norms = [str(n) for n in G[role + ".grad_names"]], G[role + ".grad_norms"]
        for n, ref in zip(names, norms):
            got = np.sqrt((grads[n] ** 2).sum())
            assert abs(got - ref) <= 3e-4 * ref + 1e-6 * norms.max(), "%s grad norm %s: %.6e vs %.6e" % (role, n, got, ref)
        pre = role + ".gslice."
        for k in G.files:
            if k.startswith(pre):
                ref, g = G[k], grads[k[len(pre):]]
                got = g[:8, :64] if ref.ndim == 2 else g
                assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-6 * norms.max(), "%s grad slice %s" % (role, k[len(pre):])


def test_lead_step_without_train_de_leaves_the_teacher_alone(dev, golden_dir):
    """train_de off: b = x = 0, the teacher forward runs without a graph, its gradient buffer is never touched."""
    from simxns_amd.LEAD.run_LEAD import lead_distill_step
    G = np.load(os.path.join(golden_dir, "lead_step_tiny.npz"))
    model_de, model_db = _models(G, dev)
    batch = [torch.from_numpy(G[k]) for k in ("q_ids", "q_mask", "d_ids", "d_mask")]
    loss, d = lead_distill_step(_args(G, train_de=False, gradient_accumulation_steps=2), model_de, model_db, batch,
                                [int(v) for v in G["sel_db"]], [int(v) for v in G["sel_teacher"]])
    torch.cuda.synchronize()
    assert "loss_dual" not in d and model_de.question_model.engine.flat_grad is None
    db, _, dis, _ = (float(v) for v in G["paras"])
    want = db * float(G["dict.loss_db"]) + dis * float(G["dict.loss_de_db_dis"]) + float(G["dict.loss_de_db_layer_dis"])
    assert abs(loss.item() - want / 2.0) <= 1e-3
    assert float(model_db.question_model.engine.flat_grad.abs().max()) > 0
