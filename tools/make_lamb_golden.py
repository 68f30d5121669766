"""Write tests/golden/lamb_trajectory.npz (+ lamb_trajectory_step<k>.npz): four steps of the IMPORTED REFERENCE's Lamb
(PROD/ProD_KD/utils/lamb.py, the class get_optimizer builds for --optimizer lamb) in float64, each after
torch.nn.utils.clip_grad_norm_(params, 1.0), with a different learning rate per step.

TEST INFRASTRUCTURE in the pattern of tools/make_kd_golden.py; it needs a checkout of the reference project (not needed to
build, test or run the package), only the .npz files travel.  Run:  python -m tools.make_lamb_golden [--reference DIR]

Six parameters in get_optimizer's two groups (decay 0.01: a, c, d, f; no decay: b, e), packed back to back in the order a..f:
  a     1 element                        the smallest segment
  b     3 elements                       starts at element offset 1: an unaligned start
  c     257, initialised to zero         weight_norm == 0 -> trust ratio 1 at step 1
  d     2 * SIMX_LAMB_CHUNK + 5          three chunks, the last one ragged (4101 when the chunk is <= 2048)
  e     768, gradient zero at every step adam_norm == 0 -> trust ratio 1, p unchanged
  f     12000 drawn at scale 0.2         |p| > 10: the clamp
The tool asserts that each of these cases really occurred, and that every step clipped (coefficient < 1).

Inputs are rounded to float32 first (and stored so), so the f32 kernels see exactly the numbers the reference saw.
lamb_trajectory.npz holds the inputs (p0 [N], g [4, N] packed), the segment table (names, seg_off, seg_len, seg_wd), lr [4],
betas, eps, weight_decay, max_norm, chunk, and per step coef [4] and stats [4, 6, 3] = weight_norm, adam_norm, trust_ratio;
lamb_trajectory_step<k>.npz holds p, m, v [N] (float64, packed) after step k -- one file per step because float64 results do
not compress and a committed file stays under 1 MiB.
"""
import argparse
import os
import re
import sys
import types
import warnings

import numpy as np
import torch

from oracle.make_golden import REF, _load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lamb_trajectory.npz")
STEPS, WD, MAX_NORM, EPS, BETAS = 4, 0.01, 1.0, 1e-6, (0.9, 0.999)
LRS = (1e-3, 2e-3, 1.5e-3, 5e-4)
GRAD_SCALE = (0.05, 0.02, 0.08, 0.03)


def chunk_size():
    hdr = open(os.path.join(ROOT, "include", "simx.h")).read()
    return int(re.search(r"#define\s+SIMX_LAMB_CHUNK\s+(\d+)", hdr).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF, help="checkout of the reference project")
    ref = ap.parse_args().reference
    warnings.simplefilter("ignore")
    # utils/lamb.py imports tensorboardX for its logging helper only: an empty stand-in serves
    if "tensorboardX" not in sys.modules:
        tbx = types.ModuleType("tensorboardX")
        tbx.SummaryWriter = type("SummaryWriter", (object,), {})
        sys.modules["tensorboardX"] = tbx
    RL = _load("ref_prod_lamb", os.path.join(ref, "PROD/ProD_KD/utils/lamb.py"))

    chunk = chunk_size()
    rs = np.random.RandomState(41)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    spec = [("a", 1, WD, 0.5), ("b", 3, 0.0, 0.5), ("c", 257, WD, 0.0), ("d", 4101 if chunk <= 2048 else 2 * chunk + 5, WD, 0.05),
            ("e", 768, 0.0, 0.3), ("f", 12000, WD, 0.2)]
    names = [s[0] for s in spec]
    init = {n: f32(rs.randn(k) * sc) for n, k, wd, sc in spec}
    grads = [{n: f32(rs.randn(k) * (0.0 if n == "e" else GRAD_SCALE[t])) for n, k, wd, sc in spec} for t in range(STEPS)]
    params = {n: torch.nn.Parameter(torch.tensor(init[n], dtype=torch.float64)) for n in names}
    groups = [{"params": [params[n] for n, k, wd, sc in spec if wd != 0.0], "weight_decay": WD},
              {"params": [params[n] for n, k, wd, sc in spec if wd == 0.0], "weight_decay": 0.0}]
    opt = RL.Lamb(groups, lr=LRS[0], eps=EPS, betas=BETAS)

    pack = lambda d: np.concatenate([np.asarray(d[n], dtype=np.float64).reshape(-1) for n in names])
    off = np.cumsum([0] + [k for n, k, wd, sc in spec])
    out = dict(names=np.array(names), seg_off=off[:-1].astype(np.int64), seg_len=np.array([s[1] for s in spec], dtype=np.int64),
               seg_wd=np.array([s[2] for s in spec], dtype=np.float64), lr=np.array(LRS, dtype=np.float64), betas=np.array(BETAS),
               eps=np.float64(EPS), weight_decay=np.float64(WD), max_norm=np.float64(MAX_NORM), chunk=np.int64(chunk),
               p0=pack(init).astype(np.float32), g=np.stack([pack(g) for g in grads]).astype(np.float32))
    coef, stats = np.zeros(STEPS), np.zeros((STEPS, len(names), 3))
    for t in range(STEPS):
        for n in names:
            params[n].grad = torch.tensor(grads[t][n], dtype=torch.float64)
        total = float(torch.nn.utils.clip_grad_norm_([params[n] for n in names], MAX_NORM))
        coef[t] = min(1.0, MAX_NORM / (total + 1e-6))
        for g in opt.param_groups:
            g["lr"] = LRS[t]
        opt.step()
        for i, n in enumerate(names):
            st = opt.state[params[n]]
            assert st["step"] == t + 1
            stats[t, i] = [float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])]
        step = dict(p=pack({n: params[n].detach().numpy() for n in names}),
                    m=pack({n: opt.state[params[n]]["exp_avg"].numpy() for n in names}),
                    v=pack({n: opt.state[params[n]]["exp_avg_sq"].numpy() for n in names}))
        assert all(np.isfinite(a).all() for a in step.values())
        path = OUT[:-4] + "_step%d.npz" % (t + 1)
        np.savez_compressed(path, **step)
        print(" step %d: |g| %.4f coef %.6f  ratios %s  -> %s (%d bytes)" % (t + 1, total, coef[t], np.round(stats[t, :, 2], 4),
                                                                          os.path.basename(path), os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20
    out.update(coef=coef, stats=stats)

    ia, ib, ic, id_, ie, if_ = range(6)
    assert (coef < 1.0).all(), "every step must clip"
    assert stats[0, ic, 0] == 0.0 and stats[0, ic, 1] > 0.0 and stats[0, ic, 2] == 1.0, "c: weight_norm == 0 -> ratio 1 at step 1"
    assert (stats[1:, ic, 0] > 0.0).all() and (stats[1:, ic, 2] != 1.0).all(), "c leaves the special case after step 1"
    assert (stats[:, ie, 1] == 0.0).all() and (stats[:, ie, 2] == 1.0).all() and (stats[:, ie, 0] > 0.0).all(), "e: adam_norm == 0 -> ratio 1"
    e = slice(off[ie], off[ie + 1])
    for t in range(STEPS):
        assert (np.load(OUT[:-4] + "_step%d.npz" % (t + 1))["p"][e] == out["p0"][e].astype(np.float64)).all(), "e stays unchanged"
    assert (stats[:, if_, 0] == 10.0).all(), "f: the clamp"
    assert (stats[:, [ia, ib, id_], 0] < 10.0).all() and (stats[:, [ia, ib, id_], 2] != 1.0).all()
    assert off[ib] % 4 != 0 and -(-spec[id_][1] // chunk) >= 3 and spec[id_][1] % chunk != 0
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
