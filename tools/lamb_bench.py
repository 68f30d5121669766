#!/usr/bin/env python
"""Time FusedAdamW.step and FusedLamb.step on one BERT-base tower's flat buffers (109.5 M f32 parameters) with HIP events.

Both optimizers step their own copy of the tower, alternately inside one loop, so that clock and neighbour noise hit both
alike; the gradients are refilled outside the timed window (a step zeroes them).  Reported per optimizer and per mode
(plain / with clip_grad_norm_, which adds the 4 B/param norm pass): median and min ms per step, and the effective rate over the
bytes the algorithm moves -- AdamW 32 B/param (16 read + 12 written + 4 zeroed), LAMB 44 B/param (pass A 16 + 8, pass B 12 + 8).
The printed line is one JSON object; --out writes it to a file as well.  Needs a GPU: there is no CPU fallback.

Run:  python tools/lamb_bench.py [--iters 30] [--warmup 5] [--layers 12] [--out profiles/lamb_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"adamw": 32, "lamb": 44}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from simxns_amd import _lib as L
    from simxns_amd.engine import BertConfigLite
    from simxns_amd.model.models import HFBertEncoder
    from simxns_amd.optim import FusedAdamW, FusedLamb
    if not torch.cuda.is_available():
        raise SystemExit("lamb_bench: no GPU (a time can only be measured on one)")
    dev = torch.device("cuda:0")
    cfg = BertConfigLite(num_hidden_layers=a.layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    towers, opts = {}, {}
    for name, cls in (("adamw", FusedAdamW), ("lamb", FusedLamb)):
        torch.manual_seed(0)
        m = HFBertEncoder(cfg, "fp32").to(dev)
        m.engine.flat.normal_(0.0, 0.02)
        m.engine.ensure_grad()
        towers[name] = m
        # (AdamW's decay of the towers is a separate elementwise pass per tensor: kept out, the kernels are what is compared)
        opts[name] = cls(m, lr=1e-4, eps=1e-6, weight_decay=a.weight_decay if name == "lamb" else 0.0)
    n = towers["lamb"].engine.flat.numel()
    times = {(k, mode): [] for k in opts for mode in ("plain", "clip")}
    for it in range(a.warmup + a.iters):
        for mode, max_norm in (("plain", 0.0), ("clip", 1.0)):
            for k in ("adamw", "lamb"):
                towers[k].engine.flat_grad.normal_(0.0, 1e-3)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                opts[k].step(max_grad_norm=max_norm)
                t1.record()
                t1.synchronize()
                if it >= a.warmup:
                    times[(k, mode)].append(t0.elapsed_time(t1))
    plan = opts["lamb"]._plan["bufs"][0]
    res = {"tool": "lamb_bench", "device": torch.cuda.get_device_name(0), "params": n, "layers": a.layers, "iters": a.iters,
           "warmup": a.warmup, "lamb_chunk": int(L.load().simx_lamb_chunk()), "lamb_segments": plan["nseg"], "lamb_chunks": plan["nchunk"]}
    for (k, mode), ts in sorted(times.items()):
        per = BYTES[k] + (4 if mode == "clip" else 0)
        med = statistics.median(ts)
        res["%s_%s" % (k, mode)] = {"bytes_per_param": per, "ms_median": round(med, 4), "ms_min": round(min(ts), 4),
                                    "ms_max": round(max(ts), 4), "tb_per_s_at_median": round(per * n / (med * 1e-3) / 1e12, 3)}
    res["lamb_over_adamw_plain"] = round(res["lamb_plain"]["ms_median"] / res["adamw_plain"]["ms_median"], 3)
    res["predicted_by_bytes"] = round(44.0 / 32.0, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
