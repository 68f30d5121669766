#!/usr/bin/env python
"""Time the LEAD distillation step at the shape of LEAD/distillation/distill_from_12de_to_6de.sh with HIP events.

BERT-base 12-layer teacher and 6-layer student, each one shared tower for queries (32 tokens) and passages (128 tokens), a batch
of 32 queries x (1 + 15) passages, 5 layer slots + the final slot, in the fp16 and the fp32 engine.  Three measurements, run
alternately inside one loop so that clock and neighbour noise hit all alike, events recorded on the launch stream:
  lead      lead_distill_step: both towers forward with [CLS] taps, the slot loss (train_de, layer_score_reweight), backward
  baseline  the same two towers, no taps, each with the existing in-batch NLL loss (ops.inbatch_nll_loss), backward
  loss      ops.lead_layer_score_loss alone (forward + the gradients, which the call produces) on ready-made vectors
The cost of taps and loss is reported as lead - baseline.  The printed line is one JSON object; --out writes it to a file as
well.  Needs a GPU: there is no CPU fallback.

Run:  python tools/lead_bench.py [--iters 10] [--warmup 3] [--dtypes fp16,fp32] [--out profiles/lead_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--neg", type=int, default=15)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from simxns_amd import ops
    from simxns_amd.engine import BertConfigLite
    from simxns_amd.LEAD.models import BiBertEncoder
    from simxns_amd.LEAD.run_LEAD import lead_distill_step
    from simxns_amd.model.models import HFBertEncoder
    from simxns_amd.utils import synth
    if not torch.cuda.is_available():
        raise SystemExit("lead_bench: no GPU (a time can only be measured on one)")
    dev = torch.device("cuda:0")
    B, C = a.batch, a.batch * (1 + a.neg)
    q_ids, q_mask, _ = synth.make_batch(901, B, 32, 30522, 9, 3, 4)
    d_ids, d_mask, _ = synth.make_batch(902, C, 128, 30522, 80, 25, 16)
    batch = [torch.from_numpy(x).to(dev) for x in (q_ids, q_mask, d_ids, d_mask)]
    pos = [i * (1 + a.neg) for i in range(B)]
    sel_db, sel_de = list(range(6 - a.slots, 6)), list(range(12 - a.slots, 12))          # layer_selection_last
    args = types.SimpleNamespace(distill_de=True, distill_db=True, train_de=True, train_db=True, distill_de_db_layer_score=True,
                                 layer_score_reweight=True, temperature=1.0, layer_temperature=10.0, distill_para_db=1.0,
                                 distill_para_de=1.0, distill_para_de_db_dis=1.0, distill_para_de_db_layer_score=1.0,
                                 gradient_accumulation_steps=1)
    res = {"tool": "lead_bench", "device": torch.cuda.get_device_name(0), "batch": B, "neg": a.neg, "layer_slots": a.slots, "q_len": 32,
           "p_len": 128, "iters": a.iters, "warmup": a.warmup, "row_kernel_launches": 3}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)
    for dtype in a.dtypes.split(","):
        models = []
        for layers, seed in ((12, 31), (6, 32)):
            cfg = BertConfigLite(num_hidden_layers=layers, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
            enc = HFBertEncoder(cfg, dtype)
            enc.load_numpy_state(synth.fill_bert_state_dict([(k, tuple(p.shape)) for k, p in enc.named_parameters()], seed))
            m = BiBertEncoder.__new__(BiBertEncoder)
            torch.nn.Module.__init__(m)
            m.question_model = m.ctx_model = enc
            models.append(m.to(dev).train())
        model_de, model_db = models
        n, H = a.slots + 1, 768
        g = torch.Generator(device=dev).manual_seed(3)
        vec = [torch.randn(n, r, H, device=dev, generator=g) * 0.3 for r in (B, C, B, C)]
        slots = [(0.0, 0.0, 0.0, 0.0, 1)] * a.slots + [(1.0, 1.0, 1.0, 1.0, 0)]

        def lead():
            lead_distill_step(args, model_de, model_db, batch, sel_db, sel_de)

        def baseline():
            for m in (model_db, model_de):
                q, c, _, _, _ = m(*batch)
                loss, _ = ops.inbatch_nll_loss(q, c, pos)
                loss.backward()

        def loss_only():
            ops.lead_layer_score_loss(*vec, pos, slots, 1.0, 10.0)
        times = {"lead": [], "baseline": [], "loss": []}
        for it in range(a.warmup + a.iters):
            for name, fn in (("lead", lead), ("baseline", baseline), ("loss", loss_only)):
                model_de.zero_grad(); model_db.zero_grad()
                ms = timed(fn)
                if it >= a.warmup:
                    times[name].append(ms)
        r = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}
        r["taps_and_loss_ms"] = round(r["lead"]["ms_median"] - r["baseline"]["ms_median"], 4)
        res[dtype] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
