"""FusedLamb without a GPU: the float64 restatement of the reference's Lamb (PROD/ProD_KD/utils/lamb.py:60-123) against the
recorded trajectory of the imported reference (tests/golden/lamb_trajectory*.npz, tools/make_lamb_golden.py), the C ABI's
declarations, both get_optimizer factories, the segment table and the checkpoint layout.  No kernel is launched here."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("weight_norm", "adam_norm", "trust_ratio")


def _lib():
    from simxns_amd import _lib as L
    L.load()
    return L


# ------------------------------------------------------------------------------------------ the restatement (shared with the GPU tests)
def clip_coef(g, max_norm, grad_scale=1.0):
    """clip_grad_norm_'s coefficient for the packed gradient `g` (in g's dtype), times grad_scale as adamw_kernel folds it."""
    T = g.dtype.type
    total = np.sqrt(np.sum(g * g, dtype=g.dtype)) * T(grad_scale)
    return T(grad_scale) * min(T(1.0), T(max_norm) / (total + T(1e-6)))


def lamb_step(p, m, v, g, segs, lr, betas, eps):
    """One Lamb step in place on the packed arrays, in their dtype; `g` is already clipped.  `segs`: [(offset, elements, weight
    decay)].  -> [(weight_norm, adam_norm, trust_ratio)] per segment."""
    T = p.dtype.type
    # (as in the reference, 1 - beta is taken in Python's float64 and only then becomes a scalar of the tensors' dtype)
    b1, b2, c1, c2 = T(betas[0]), T(betas[1]), T(1.0 - float(betas[0])), T(1.0 - float(betas[1]))
    out = []
    for off, n, wd in segs:
        s = slice(int(off), int(off) + int(n))
        m[s] = b1 * m[s] + c1 * g[s]
        v[s] = b2 * v[s] + c2 * g[s] * g[s]
        u = m[s] / (np.sqrt(v[s]) + T(eps)) + T(wd) * p[s]
        wn = min(np.sqrt(np.sum(p[s] * p[s], dtype=p.dtype)), T(10.0))
        an = np.sqrt(np.sum(u * u, dtype=p.dtype))
        r = T(1.0) if wn == 0 or an == 0 else wn / an
        p[s] = p[s] - T(lr) * r * u
        out.append((wn, an, r))
    return out


def load_trajectory(golden_dir):
    G = dict(np.load(os.path.join(golden_dir, "lamb_trajectory.npz")))
    G["steps"] = [dict(np.load(os.path.join(golden_dir, "lamb_trajectory_step%d.npz" % (t + 1)))) for t in range(len(G["lr"]))]
    G["segs"] = list(zip(G["seg_off"].tolist(), G["seg_len"].tolist(), G["seg_wd"].tolist()))
    return G


def restate(G, dtype, grad_mul=1.0, grad_scale=1.0):
    """The whole trajectory in `dtype` from the fixture's f32 inputs -> per step (p, m, v, stats, coef)."""
    p = G["p0"].astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for t in range(len(G["lr"])):
        g = G["g"][t].astype(dtype) * dtype(grad_mul)
        c = clip_coef(g, float(G["max_norm"]), grad_scale)
        stats = lamb_step(p, m, v, g * c, G["segs"], G["lr"][t], G["betas"], float(G["eps"]))
        out.append((p.copy(), m.copy(), v.copy(), np.array(stats, dtype=np.float64), float(c)))
    return out


@pytest.fixture(scope="module")
def G(golden_dir):
    return load_trajectory(golden_dir)


def test_fixture_regenerates_from_float64_restatement(G):
    L = _lib()
    assert int(G["chunk"]) == L.load().simx_lamb_chunk(), "regenerate the fixture: parameter d spans 2 chunks + 5 elements"
    assert G["names"].tolist() == list("abcdef") and G["seg_len"].tolist()[:3] == [1, 3, 257] and G["seg_len"].tolist()[4:] == [768, 12000]
    assert G["seg_len"][3] == (4101 if G["chunk"] <= 2048 else 2 * G["chunk"] + 5)
    assert G["p0"].dtype == np.float32 and G["g"].dtype == np.float32 and len(G["steps"]) == 4
    for t, (p, m, v, stats, coef) in enumerate(restate(G, np.float64)):
        ref = G["steps"][t]
        for k, a in (("p", p), ("m", m), ("v", v)):
            err = np.abs(a - ref[k]).max()
            assert err <= 1e-12, "step %d %s: %.3e" % (t + 1, k, err)
        assert np.abs(stats - G["stats"][t]).max() <= 1e-12 and abs(coef - G["coef"][t]) <= 1e-12
        assert coef < 1.0
    ic, ie, if_ = 2, 4, 5
    assert G["stats"][0, ic, 0] == 0.0 and G["stats"][0, ic, 2] == 1.0          # weight_norm == 0
    assert (G["stats"][:, ie, 1] == 0.0).all() and (G["stats"][:, ie, 2] == 1.0).all()   # adam_norm == 0
    assert (G["stats"][:, if_, 0] == 10.0).all()                                # the clamp


def test_header_declares_and_library_exports_lamb():
    L = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simx.h")).read(), flags=re.S)
    for name in ("simx_lamb_step", "simx_lamb_chunk"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L.load(), name) and name in L.SIGNATURES
    chunk = L.load().simx_lamb_chunk()
    assert chunk == int(re.search(r"#define\s+SIMX_LAMB_CHUNK\s+(\d+)", hdr).group(1)) and chunk >= 256 and chunk % 4 == 0


def _tiny_reranker():
    from simxns_amd.engine import BertConfigLite
    from simxns_amd.model.models import HFBertEncoder, Reranker
    cfg = BertConfigLite(vocab_size=60, hidden_size=8, num_hidden_layers=2, num_attention_heads=2, intermediate_size=16,
                         max_position_embeddings=16)
    torch.manual_seed(0)
    return Reranker(HFBertEncoder(cfg, "fp32"), 8)


def test_get_optimizer_dispatch():
    _lib()
    from simxns_amd.co_training.co_training_marco_train import get_optimizer as get_marco
    from simxns_amd.optim import FusedAdamW, FusedLamb
    from simxns_amd.ProD_KD.utils.dpr_utils import get_optimizer as get_prod
    model = _tiny_reranker()
    for name, cls in (("adamW", FusedAdamW), ("lamb", FusedLamb)):
        args = types.SimpleNamespace(optimizer=name, adam_epsilon=3e-7)
        o = get_prod(args, model, lr=2e-4, weight_decay=0.01)
        assert type(o) is cls and o.eps == 3e-7 and o.lr == 2e-4 and o.wd == 0.01
        o = get_marco(args, model, 0.01, 2e-4, 3e-7)
        assert type(o) is cls and o.eps == 3e-7 and o.lr == 2e-4 and o.wd == 0.01
    args = types.SimpleNamespace(optimizer="sgd", adam_epsilon=1e-8)
    for get in (get_prod, lambda a, m: get_marco(a, m, 0.0, 1e-5, 1e-8)):
        with pytest.raises(Exception, match="optimizer sgd not recognized! Can only be lamb or adamW"):
            get(args, model)


def test_segment_table_of_a_tiny_model():
    L = _lib()
    from simxns_amd.optim import FusedLamb, lamb_chunk_plan
    model = _tiny_reranker()
    opt = FusedLamb(model, lr=1e-3, weight_decay=0.01)
    segs = opt.segments()
    named = dict(model.named_parameters())
    stepping = [n for n in named if ".pooler." not in n]
    assert len(stepping) == len(named) - 2
    assert sorted(s[0] for s in segs) == sorted(stepping) and len(set(s[0] for s in segs)) == len(segs)
    by = {s[0]: s for s in segs}
    for n in stepping:
        assert by[n][3] == named[n].numel() and by[n][5] is named[n]
        assert by[n][4] == (0.0 if ("bias" in n or "LayerNorm.weight" in n) else 0.01), n
    # the fused QKV slot is three segments, back to back, each one [H, H] tensor of the module
    q, k, v = (by["encoder.encoder.layer.1.attention.self.%s.weight" % x] for x in ("query", "key", "value"))
    assert q[3] == k[3] == v[3] == 64 and k[2] == q[2] + 64 and v[2] == k[2] + 64 and q[1] == k[1] == v[1] == 0
    # a segment is where the parameter's storage is: a write through the flat buffer shows in the module's tensor
    e = opt.towers[0][1]
    for n in stepping:
        name, b, off, cnt, wd, p = by[n]
        if b == 0:
            assert p.data_ptr() == e.flat.data_ptr() + 4 * off, n
    # the packed extras: Linear(H, 1) weight then its one-element bias, back to back (the bias starts unaligned or not at all)
    w, bias = by["qa_classifier.weight"], by["qa_classifier.bias"]
    assert w[1] == bias[1] == 1 and w[2] == 0 and bias[2] == w[3] and bias[3] == 1 and bias[4] == 0.0
    # the plan a buffer's segments give: chunks never cross a segment and pass the library's own check
    chunk = 16
    mine = [(s[2], s[3], s[4]) for s in segs if s[1] == 0]
    assert mine == sorted(mine), "the plan wants a buffer's segments ascending; HF registration order is not (q.bias sits behind v.weight)"
    chunks, seg_chunks, seg_range, seg_wd = lamb_chunk_plan(mine, chunk)
    assert chunks.dtype.itemsize == 16 and len(seg_chunks) == len(mine) and int(seg_chunks[:, 1].sum()) == len(chunks)
    for c in chunks:
        off, n, wd = mine[c["seg"]]
        assert off <= c["off"] and c["off"] + c["len"] <= off + n and 1 <= c["len"] <= chunk
    assert int(chunks["len"].sum()) == sum(n for off, n, wd in mine)
    real = lamb_chunk_plan(mine, L.load().simx_lamb_chunk())
    hp = lambda a: a.ctypes.data_as(L.C.c_void_p)
    n = e.flat.numel()
    L.call("simx_lamb_plan_check", hp(real[0]), len(real[0]), hp(real[1]), hp(real[2]), len(mine), n)
    bad = real[0].copy()
    bad["len"][0] += 1                               # the first chunk now reaches into the next segment
    with pytest.raises(L.SimxError, match="crosses or leaves"):
        L.call("simx_lamb_plan_check", hp(bad), len(bad), hp(real[1]), hp(real[2]), len(mine), n)
    with pytest.raises(L.SimxError):
        L.call("simx_lamb_plan_check", hp(real[0]), len(real[0]), hp(real[1]), hp(real[2]), 0, n)
    with pytest.raises(L.SimxError):
        L.call("simx_lamb_plan_check", None, len(real[0]), hp(real[1]), hp(real[2]), len(mine), n)
    with pytest.raises(L.SimxError):                 # a buffer shorter than the last segment
        L.call("simx_lamb_plan_check", hp(real[0]), len(real[0]), hp(real[1]), hp(real[2]), len(mine), mine[-1][0])


def test_plan_of_a_tiny_model_passes_the_library_check():
    """FusedLamb's own plan (what step() builds before its first launch) for a model whose tensors live in host memory: the
    tables of both buffers pass simx_lamb_plan_check, every stepping parameter has one stats row, and a change in which extra
    parameters carry a gradient rebuilds the plan."""
    L = _lib()
    from simxns_amd.optim import FusedLamb
    model = _tiny_reranker()
    opt = FusedLamb(model, lr=1e-3, weight_decay=0.01)
    cpu = torch.device("cpu")
    plan = opt._plan_for(cpu)                        # no extra parameter has a gradient yet: the tower alone
    named = dict(model.named_parameters())
    tower = [n for n in named if n.startswith("encoder.") and ".pooler." not in n]
    assert [s[0] for s in plan["segs"]] != tower and sorted(s[0] for s in plan["segs"]) == sorted(tower)
    assert plan["bufs"][1] is None and plan["bufs"][0]["nseg"] == len(tower) and tuple(plan["stats"].shape) == (len(tower), 3)
    assert opt._plan_for(cpu) is plan
    for p in opt.extra:
        p.grad = torch.zeros_like(p)
    plan2 = opt._plan_for(cpu)
    assert plan2 is not plan and plan2["bufs"][1]["nseg"] == 2 and plan2["bufs"][1]["nchunk"] == 2
    assert len(plan2["segs"]) == len(tower) + 2 and tuple(plan2["stats"].shape) == (len(tower) + 2, 3)
    chunk = L.load().simx_lamb_chunk()
    assert plan2["bufs"][0]["nchunk"] == sum((named[n].numel() + chunk - 1) // chunk for n in tower)
    assert plan2["partials"].numel() == 2 * plan2["bufs"][0]["nchunk"]


def test_lamb_step_argument_checks():
    """Null pointers, n == 0 and nseg < 1 are refused before anything is launched (host pointers serve: nothing reads them)."""
    L = _lib()
    a = np.zeros(64, np.float32)
    ok = L.C.c_void_p(a.ctypes.data)
    good = [None, ok, ok, ok, ok, 16, ok, 1, ok, ok, 1, ok, ok, 1e-3, 0.9, 0.999, 1e-6, None, 0.0, 1.0, 1, None]
    for i, val in [(j, None) for j in (1, 2, 3, 4, 6, 8, 9, 11, 12)] + [(5, 0), (10, 0), (7, 0)]:
        args = list(good)
        args[i] = val
        with pytest.raises(L.SimxError):
            L.call("simx_lamb_step", *args)


def _lamb_dict(opt, step=2, seed=3):
    """What torch.optim.Optimizer.state_dict() gives for the reference's Lamb on this model after `step` steps."""
    order = opt._ref_param_order()
    rs = np.random.RandomState(seed)
    state = {}
    for i, (n, p, g) in enumerate(order):
        if ".pooler." in n:                          # grad is None: the reference never creates its state
            continue
        state[i] = {"step": step, "exp_avg": torch.from_numpy(rs.randn(*p.shape).astype(np.float32)),
                    "exp_avg_sq": torch.from_numpy(rs.rand(*p.shape).astype(np.float32)),
                    "weight_norm": torch.tensor(float(rs.rand()) * 10), "adam_norm": torch.tensor(float(rs.rand()) + 0.1),
                    "trust_ratio": torch.tensor(float(rs.rand()))}
    n0 = sum(1 for _, _, g in order if g == 0)
    base = dict(lr=7e-4, betas=(0.9, 0.999), eps=1e-6)
    return {"state": state, "param_groups": [dict(base, weight_decay=0.01, params=list(range(n0))),
                                             dict(base, weight_decay=0.0, params=list(range(n0, len(order))))]}


def test_state_dict_layout_and_round_trip():
    _lib()
    from simxns_amd.optim import FusedAdamW, FusedLamb
    model = _tiny_reranker()
    opt = FusedLamb(model, lr=1e-3, eps=1e-6, weight_decay=0.01)
    sd = opt.state_dict()
    order = opt._ref_param_order()
    n0 = sum(1 for n, p in model.named_parameters() if not ("bias" in n or "LayerNorm.weight" in n))
    assert sd["state"] == {} and "loss_scaler" not in sd and len(sd["param_groups"]) == 2
    assert [g["params"] for g in sd["param_groups"]] == [list(range(n0)), list(range(n0, len(order)))]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.01, 0.0]
    for g in sd["param_groups"]:
        assert g["lr"] == 1e-3 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-6 and "correct_bias" not in g
    # a Lamb-shaped dict round-trips
    ref = _lamb_dict(opt)
    opt.load_state_dict(ref)
    assert opt.step_count == 2 and opt.param_groups[0]["lr"] == 7e-4
    out = opt.state_dict()
    assert set(out["state"]) == set(ref["state"]) and len(ref["state"]) == len(order) - 2
    for i, st in ref["state"].items():
        assert set(out["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} | set(SCALARS)
        assert out["state"][i]["step"] == 2
        for k in ("exp_avg", "exp_avg_sq") + SCALARS:
            assert torch.equal(out["state"][i][k], st[k]), (order[i][0], k)
    assert [g["params"] for g in out["param_groups"]] == [g["params"] for g in ref["param_groups"]]
    assert all(g["lr"] == 7e-4 for g in out["param_groups"])
    # ... and into a fresh optimizer, whose dict is the same again
    opt2 = FusedLamb(_tiny_reranker(), lr=1e-3, weight_decay=0.01)
    opt2.load_state_dict(out)
    out2 = opt2.state_dict()
    for i in out["state"]:
        for k in ("exp_avg", "exp_avg_sq") + SCALARS:
            assert torch.equal(out2["state"][i][k], out["state"][i][k])
    # an AdamW-shaped dict: the moments carry over, the three scalars wait for the next step; the pooler slots stay stateless
    adam = FusedAdamW(model, lr=1e-3, weight_decay=0.01)
    adam.load_state_dict({"state": {i: {k: v for k, v in st.items() if k not in SCALARS} for i, st in ref["state"].items()},
                          "param_groups": ref["param_groups"]})
    asd = adam.state_dict()
    assert len(asd["state"]) == len(order)
    opt3 = FusedLamb(model, lr=1e-3, weight_decay=0.01)
    opt3.load_state_dict(asd)
    out3 = opt3.state_dict()
    assert set(out3["state"]) == set(ref["state"])
    for i, st in ref["state"].items():
        assert set(out3["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(out3["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(out3["state"][i]["exp_avg_sq"], st["exp_avg_sq"])
    # another parameter count or shape is an error
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [{"params": [0, 1]}]})
    wrong = _lamb_dict(opt)
    wrong["state"][0]["exp_avg"] = torch.zeros(3, 5)
    with pytest.raises(ValueError):
        opt.load_state_dict(wrong)
