"""simx_lamb_step and FusedLamb on the GPU: the recorded float64 trajectory of the imported reference's Lamb
(tests/golden/lamb_trajectory*.npz) through the C ABI, grad_scale, the loss scaler's skip, bit reproducibility, and the class
end to end on a tiny bi-encoder, in the distillation step and across a checkpoint.

Tolerance: rtol 1e-5, atol 1e-6 on p, m, v (what test_adamw_clip holds AdamW to), rtol 1e-5 on the three scalars.  The same
update restated in float32 NumPy on the fixture's inputs stays within 0.016 of that bound on p and 0.0005 on m (asserted below at
0.02, on the CPU; its scalars are within 1.3e-7 relative), so the bound leaves the kernels' other summation order fifty-fold room."""
import math
import types

import numpy as np
import pytest
import torch

from test_lamb_cpu import clip_coef, lamb_step, load_trajectory, restate

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6


def L():
    from simxns_amd import _lib
    _lib.load()
    return _lib


def _within(got, ref, what, rtol=RTOL, atol=ATOL):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, bound = np.abs(got - ref), atol + rtol * np.abs(ref)
    assert (err[bound == 0.0] == 0.0).all(), "%s: a reference of exactly 0 is not met exactly" % what
    worst = (err[bound > 0.0] / bound[bound > 0.0]).max() if (bound > 0.0).any() else 0.0
    print("%s: %.4f of the bound" % (what, worst))
    assert worst <= 1.0, "%s: %.3f of the bound (rtol %g, atol %g)" % (what, worst, rtol, atol)
    return worst


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


@pytest.fixture(scope="module")
def G(golden_dir):
    return load_trajectory(golden_dir)


class Flat(object):
    """The fixture's packed buffer on the device with its plan, stepped through simx_lamb_step."""

    def __init__(self, G, dev):
        from simxns_amd.optim import lamb_chunk_plan
        lib = L()
        self.lib, self.G, self.dev = lib, G, dev
        self.n = int(G["p0"].size)
        chunks, seg_chunks, seg_range, seg_wd = lamb_chunk_plan(G["segs"], lib.load().simx_lamb_chunk())
        hp = lambda a: a.ctypes.data_as(lib.C.c_void_p)
        lib.call("simx_lamb_plan_check", hp(chunks), len(chunks), hp(seg_chunks), hp(seg_range), len(G["segs"]), self.n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        self.nchunk, self.nseg = len(chunks), len(G["segs"])
        assert int(seg_chunks[3, 1]) == 3 and int(chunks["off"][1]) % 4 == 1       # d: three chunks; b: an unaligned start
        self.chunks, self.seg_chunks, self.seg_wd = up(chunks), up(seg_chunks), up(seg_wd)
        self.p = torch.from_numpy(G["p0"].copy()).to(dev)
        self.g, self.m, self.v = (torch.zeros(self.n, dtype=torch.float32, device=dev) for _ in range(3))
        self.stats = torch.full((self.nseg, 3), float("nan"), dtype=torch.float32, device=dev)
        self.partials = torch.zeros(2 * self.nchunk, dtype=torch.float32, device=dev)
        self.ws = torch.empty(2048, dtype=torch.float32, device=dev)

    def step(self, t, grad_mul=1.0, grad_scale=1.0, scaler=None, zero_grad=1):
        lib, G = self.lib, self.G
        self.g.copy_(torch.from_numpy(G["g"][t] * np.float32(grad_mul)))
        sq = torch.zeros(1, dtype=torch.float32, device=self.dev)
        lib.call("simx_sqnorm_accum_det", lib.stream_ptr(), lib.ptr(self.g), self.n, lib.ptr(sq), lib.ptr(self.ws))
        lib.call("simx_lamb_step", lib.stream_ptr(), lib.ptr(self.p), lib.ptr(self.g), lib.ptr(self.m), lib.ptr(self.v), self.n,
                 lib.ptr(self.chunks), self.nchunk, lib.ptr(self.seg_chunks), lib.ptr(self.seg_wd), self.nseg, lib.ptr(self.stats),
                 lib.ptr(self.partials), float(G["lr"][t]), float(G["betas"][0]), float(G["betas"][1]), float(G["eps"]), lib.ptr(sq),
                 float(G["max_norm"]), grad_scale, zero_grad, lib.ptr(scaler))
        torch.cuda.synchronize()
        return sq

    def host(self):
        return tuple(a.detach().cpu().numpy().copy() for a in (self.p, self.m, self.v, self.stats))


def _run(G, dev, **kw):
    f = Flat(G, dev)
    out = []
    for t in range(len(G["lr"])):
        f.step(t, **kw)
        out.append(f.host() + (f.g.detach().cpu().numpy().copy(),))
    return out


@pytest.fixture(scope="module")
def run(G, dev):
    return _run(G, dev)


def _check_against_reference(G, run, what):
    ic, ie, if_ = 2, 4, 5
    for t, (p, m, v, stats, g) in enumerate(run):
        ref = G["steps"][t]
        for k, a in (("p", p), ("m", m), ("v", v)):
            _within(a, ref[k], "%s step %d %s" % (what, t + 1, k))
        _within(stats, G["stats"][t], "%s step %d stats" % (what, t + 1), atol=0.0)
        assert np.abs(g).max() == 0.0, "gradients are zeroed in the same pass"
        assert stats[ie, 2] == 1.0 and stats[ie, 1] == 0.0, "adam_norm == 0 -> trust ratio exactly 1"
        assert stats[if_, 0] == 10.0, "the clamp: weight_norm exactly 10"
        e = slice(int(G["seg_off"][ie]), int(G["seg_off"][ie] + G["seg_len"][ie]))
        assert (p[e] == G["p0"][e]).all(), "a parameter whose update is zero keeps its bits"
    assert run[0][3][ic, 2] == 1.0 and run[0][3][ic, 0] == 0.0, "weight_norm == 0 -> trust ratio exactly 1"


def test_trajectory_against_reference(G, run):
    # the tolerance's footing: the update restated in f32 on the CPU uses a fiftieth of the bound
    for t, (p, m, v, stats, coef) in enumerate(restate(G, np.float32)):
        ref = G["steps"][t]
        for k, a in (("p", p), ("m", m), ("v", v)):
            worst = (np.abs(a.astype(np.float64) - ref[k]) / (ATOL + RTOL * np.abs(ref[k]))).max()
            print("f32 restatement step %d %s: %.4f of the bound" % (t + 1, k, worst))
            assert worst <= 0.02
    _check_against_reference(G, run, "lamb")


def test_grad_scale_folds_into_the_update(G, dev):
    """Every gradient doubled (the sum over two ranks) and grad_scale = 0.5 (the DDP mean): the same trajectory."""
    _check_against_reference(G, _run(G, dev, grad_mul=2.0, grad_scale=0.5), "grad_scale 0.5")


def test_scaler_skip_keeps_every_bit(G, dev):
    f = Flat(G, dev)
    f.step(0)
    before = [_bits(a) for a in (f.p, f.m, f.v, f.stats)]
    sc = torch.tensor([65536.0, 1.0 / 65536.0, 0.0, 1.0, 1.0, 1.0, 2000.0, 2.0 ** 24], dtype=torch.float32, device=dev)
    f.step(1, scaler=sc)
    for a, b, k in zip(before, [_bits(a) for a in (f.p, f.m, f.v, f.stats)], "p m v stats".split()):
        assert (a == b).all(), "a skipped step changed %s" % k
    assert float(f.g.abs().max()) == 0.0, "a skipped step still drops its gradients"
    sc[3] = 0.0
    f.step(1, scaler=sc)
    plain = Flat(G, dev)
    plain.step(0)
    plain.step(1)
    for a, b, k in zip(f.host(), plain.host(), "p m v stats".split()):
        assert (a.view(np.int32) == b.view(np.int32)).all(), "with the flag cleared the step applies as without a scaler (%s)" % k
    assert (before[0] != _bits(f.p)).any()


def test_two_runs_give_the_same_bits(G, dev, run):
    again = _run(G, dev)
    for t, (a, b) in enumerate(zip(run, again)):
        assert (a[0].view(np.int32) == b[0].view(np.int32)).all(), "p differs at step %d" % (t + 1)
        assert (a[3].view(np.int32) == b[3].view(np.int32)).all(), "stats differ at step %d" % (t + 1)


# ------------------------------------------------------------------------------------------ the class
def _cfg():
    from simxns_amd.engine import BertConfigLite
    return BertConfigLite(vocab_size=200, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                          max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _encoder(seed):
    from oracle.weights import BertCfg, make_bert_params
    from simxns_amd.ProD_KD.model.models import HFBertEncoder
    m = HFBertEncoder(_cfg(), compute_dtype="fp32")
    m.load_numpy_state(make_bert_params(BertCfg(vocab=200, hidden=32, layers=2, heads=2, inter=64, max_pos=64), seed, std=0.08))
    return m


def _bi(dev, sq=1, sc=2):
    from simxns_amd.ProD_KD.model.models import BiBertEncoder
    m = BiBertEncoder.__new__(BiBertEncoder)
    torch.nn.Module.__init__(m)
    m.question_model, m.ctx_model = _encoder(sq), _encoder(sc)
    return m.to(dev)


def _batch(dev, seed=0):
    from oracle.weights import make_batch
    B, N = 3, 3
    t = lambda a: torch.from_numpy(a).to(dev)
    q_ids, q_mask, _ = make_batch(21 + seed, B, 16, 200, 9, 3, 4)
    c_ids, c_mask, _ = make_batch(22 + seed, B * (1 + N), 32, 200, 20, 6, 8)
    z = np.linspace(-2, 2, B * (1 + N)).reshape(B, 1 + N).astype(np.float32)
    return t(q_ids), t(q_mask), t(c_ids), t(c_mask), t(z)


def _backward(model, batch):
    from simxns_amd import ops
    q_ids, q_mask, c_ids, c_mask, z = batch
    q, c = model(q_ids, q_mask, c_ids, c_mask)
    loss, _, _ = ops.kl_distill_loss(q, c, z)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss)


def test_fused_lamb_end_to_end(dev):
    from simxns_amd.optim import FusedLamb
    model = _bi(dev)
    model.train()
    opt = FusedLamb(model, lr=2e-3, eps=1e-6, weight_decay=0.01)
    named = dict(model.named_parameters())
    stepping = [n for n in named if ".pooler." not in n]
    assert len(stepping) == len(named) - 4
    M = {n: np.zeros(named[n].numel()) for n in stepping}
    V = {n: np.zeros(named[n].numel()) for n in stepping}
    for it in range(2):                               # (the second step runs on non-zero moments)
        _backward(model, _batch(dev, it))
        P = {n: p.detach().cpu().numpy().astype(np.float64).reshape(-1) for n, p in named.items()}
        Gr = {n: p.grad.detach().cpu().numpy().astype(np.float64).reshape(-1) for n, p in named.items()}
        assert all(np.abs(Gr[n]).max() == 0.0 for n in named if ".pooler." in n)
        assert sum(1 for n in stepping if np.abs(Gr[n]).max() > 0) > 30
        pool_bits = {n: _bits(named[n]) for n in named if ".pooler." in n}
        coef = clip_coef(np.concatenate([Gr[n] for n in named]), 2.0)
        opt.step(max_grad_norm=2.0)
        torch.cuda.synchronize()
        ratios = opt.trust_ratios()
        assert sorted(ratios) == sorted(stepping)
        for n in stepping:
            wd = 0.0 if ("bias" in n or "LayerNorm.weight" in n) else 0.01
            (wn, an, r), = lamb_step(P[n], M[n], V[n], Gr[n] * coef, [(0, P[n].size, wd)], 2e-3, (0.9, 0.999), 1e-6)
            _within(named[n].detach().cpu().numpy().reshape(-1), P[n], "step %d %s" % (it + 1, n))
            _within(ratios[n], (wn, an, r), "step %d %s scalars" % (it + 1, n), atol=0.0)
        for n, b in pool_bits.items():
            assert (_bits(named[n]) == b).all(), "%s is in no segment and keeps its bits, also under weight decay" % n
        for n, p in named.items():
            assert float(p.grad.abs().max()) == 0.0, n
    sd = opt.state_dict()
    assert len(sd["state"]) == len(stepping) and all(st["step"] == 2 and "trust_ratio" in st for st in sd["state"].values())


def test_distill_step_with_fused_lamb(dev):
    from oracle.weights import make_batch
    from simxns_amd.optim import FusedLamb, LinearWarmupSchedule
    from simxns_amd.ProD_KD.model.models import Reranker
    from simxns_amd.ProD_KD.run_progressive_distill_marco import cross_encoder_distill_step
    from simxns_amd.ProD_KD.utils.dpr_utils import get_optimizer
    model, teacher = _bi(dev), Reranker(_encoder(5), 32).to(dev)
    opt = get_optimizer(types.SimpleNamespace(optimizer="lamb", adam_epsilon=1e-6), model, lr=1e-3, weight_decay=0.01)
    assert type(opt) is FusedLamb
    sched = LinearWarmupSchedule(opt, 1, 4)
    B, N = 3, 3
    t = lambda a: torch.from_numpy(a).to(dev)
    args = types.SimpleNamespace(KD_type="KD_softmax", TEMPERATURE=4.0, CE_WEIGHT=0.1, KD_WEIGHT=0.9, LwF_WEIGHT=1.0, DKD_alpha=1.0,
                                 DKD_beta=8.0, open_LwF=False, gradient_accumulation_steps=1, max_grad_norm=2.0)
    model.train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    sched.step()                                      # (past the zero learning rate of warm-up step 0)
    for it in range(2):
        q_ids, q_mask, c_ids, c_mask, _ = _batch(dev, it)
        x_ids, x_mask, _ = make_batch(23 + it, B * (1 + N), 48, 200, 30, 8, 12)
        loss, _ = cross_encoder_distill_step(
            args, model, teacher, dict(query_ids=q_ids, attention_mask_q=q_mask, input_ids_a=c_ids, attention_mask_a=c_mask),
            dict(input_ids=t(x_ids).view(B, 1 + N, -1), attention_mask=t(x_mask).view(B, 1 + N, -1)), optimizer=opt, scheduler=sched)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item())
    moved = [n for n, p in model.named_parameters() if not torch.equal(p, before[n])]
    # (every decayed tensor moves; a no-decay vector whose gradient is exactly zero -- the key biases' can be -- has u = 0)
    decayed = [n for n in before if ".pooler." not in n and "bias" not in n and "LayerNorm.weight" not in n]
    assert set(decayed) <= set(moved) and len(decayed) > 20 and not any(".pooler." in n for n in moved)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert sched.t == 3 and len(opt.trust_ratios()) == len(before) - 4


def test_checkpoint_resumes_bit_identically(dev):
    from simxns_amd.optim import FusedLamb
    a = _bi(dev)
    a.train()
    oa = FusedLamb(a, lr=2e-3, weight_decay=0.01)
    for it in range(2):
        _backward(a, _batch(dev, it))
        oa.step(max_grad_norm=2.0)
    sd = oa.state_dict()
    b = _bi(dev, 7, 8)                                # other weights: everything must come from the checkpoint
    b.train()
    b.load_state_dict(a.state_dict())
    ob = FusedLamb(b, lr=1e-5, weight_decay=0.01)
    ob.load_state_dict(sd)
    assert ob.step_count == 2 and ob.param_groups[0]["lr"] == 2e-3
    _backward(a, _batch(dev, 2))
    for (ma, ea), (mb, eb) in zip(oa.towers, ob.towers):      # the same gradients into both
        assert torch.equal(ea.flat, eb.flat)
        eb.ensure_grad().copy_(ea.flat_grad)
    oa.step(max_grad_norm=2.0)
    ob.step(max_grad_norm=2.0)
    torch.cuda.synchronize()
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert (_bits(pa) == _bits(pb)).all(), n
    ra, rb = oa.trust_ratios(), ob.trust_ratios()
    assert ra == rb and len(ra) == len(list(a.named_parameters())) - 4
    sa, sb = oa.state_dict(), ob.state_dict()
    for i in sa["state"]:
        assert sb["state"][i]["step"] == 3 and torch.equal(sa["state"][i]["exp_avg_sq"], sb["state"][i]["exp_avg_sq"])
