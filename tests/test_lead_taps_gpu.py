"""GPU: the encoder's [CLS] taps (simx_bert_fwd_taps / simx_bert_bwd_taps, BertEngine.encode(tap_layers=...)).

A tap on layer l is the [CLS] embedding of the same tower cut after l + 1 layers, and by linearity the backward of
(cls . d + sum_k taps[k] . d_k) is the plain backward for d plus the truncated towers' backwards for d_k, tensor by tensor.
The truncated towers come from the same name-keyed state (synth.fill_bert_state_dict) and, with dropout, see the same
stateless masks for the layers they have (same seed, same call count, masks keyed by layer / site / row).
"""
import os

import numpy as np
import pytest
import torch

from test_encoder_gpu import _cfg_from, _named_shapes

pytestmark = pytest.mark.gpu

LAYERS, TAPS = 4, [0, 2, 3]            # first, middle, last
# The truncated tower runs its last layer in the [CLS]-only form, the tapped tower runs that layer in the full form.
#   forward : the bound tests/test_encoder_gpu.py::test_full_size_config2_properties holds "[CLS]-only vs all rows" to, of the
#             embeddings' scale.
#   backward: no existing bound covers the gradients of the two forms, so it is twice their measured disagreement -- the SAME
#             reference sum below computed with SIMX_FULL_LAST_LAYER=1 against =0, no taps involved, of the largest gradient:
#             TWO_FORMS -- plus, fp32, the 5e-6 that test_gradient_checkpointing_and_ranged_backward_change_nothing allows
#             for the atomics' summation order.  Measured on an MI355X with reference() below: fp32 3.545e-6 (dropout 0) and
#             3.492e-6 (dropout 0.1), fp16 5.138e-4, each at an embedding table (every token's gradient lands there); the same
#             form run twice differs by 4e-7 / 6e-7.  The taps themselves came out at 5.6e-6 / 5.8e-6 (fp32) and 9.5e-4 (fp16).
TOL_FWD = {"fp32": 2e-5, "fp16": 5e-3}
TWO_FORMS = {("fp32", 0.0): 3.545e-6, ("fp16", 0.0): 5.138e-4, ("fp32", 0.1): 3.492e-6}
ATOMICS = {"fp32": 5e-6, "fp16": 0.0}


def _tower(G, dev, dtype, dropout, layers, ckpt=False):
    from simxns_amd.model.models import HFBertEncoder
    from simxns_amd.utils import synth
    cfg = _cfg_from(G)
    cfg.num_hidden_layers = layers
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = dropout
    cfg.gradient_checkpointing = ckpt
    enc = HFBertEncoder(cfg, compute_dtype=dtype)
    enc.load_numpy_state(synth.fill_bert_state_dict(_named_shapes(enc), 77, std=0.08))
    enc.to(dev).train()
    enc.engine.dropout_seed = 123
    return enc


def _inputs(G, dev):
    ids, mask = torch.from_numpy(G["c_ids"]).to(dev), torch.from_numpy(G["c_mask"]).to(dev)
    rs = np.random.RandomState(3)
    H = int(_cfg_from(G).hidden_size)
    d = [torch.from_numpy(rs.randn(ids.shape[0], H).astype(np.float32)).to(dev) for _ in range(1 + len(TAPS))]
    return ids, mask, d[0], d[1:]


def _grads(enc):
    torch.cuda.synchronize()
    return {k: p.grad.detach().cpu().numpy().astype(np.float64).copy() for k, p in enc.named_parameters()}


def reference(G, dev, dtype, dropout):
    """(embeddings of the towers cut after l + 1 layers for l in TAPS, the 4-layer tower's embedding, the summed gradient)."""
    ids, mask, d, dk = _inputs(G, dev)
    embs, total = [], None
    for depth, up in [(LAYERS, d)] + [(l + 1, g) for l, g in zip(TAPS, dk)]:
        enc = _tower(G, dev, dtype, dropout, depth)
        e = enc.embed(ids, mask)
        (e * up).sum().backward()
        embs.append(e.detach().cpu().numpy())
        g = _grads(enc)
        if total is None:
            total = g
        else:
            for k, v in g.items():
                total[k] += v
    return embs[1:], embs[0], total


_REF = {}


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "step_tiny.npz"))


def _ref(G, dev, dtype, dropout):
    if (dtype, dropout) not in _REF:
        _REF[(dtype, dropout)] = reference(G, dev, dtype, dropout)
    return _REF[(dtype, dropout)]


@pytest.mark.parametrize("dtype,dropout,ckpt,parts,full_last", [
    ("fp32", 0.0, False, 1, False), ("fp16", 0.0, False, 1, False), ("fp32", 0.1, False, 1, False), ("fp32", 0.0, True, 1, False),
    ("fp16", 0.0, True, 1, False), ("fp32", 0.0, False, 3, False), ("fp32", 0.0, False, 1, True)])
def test_taps_forward_and_backward(dev, G, monkeypatch, dtype, dropout, ckpt, parts, full_last):
    """full_last: the tapped tower computes every row of its last layer (SIMX_FULL_LAST_LAYER=1), so the embedding gradient,
    joined with the last layer's tap, enters the stack through the scatter instead of the [CLS]-only layer (fp32: 6.0e-6
    measured).  There is no fp16 case of it: the reference's 4-layer towers then run the OTHER last-layer form as well, a
    third two-forms term that the bound above does not price -- measured 1.134e-3 against its 1.028e-3 (9.5e-4 in the
    [CLS]-only form), all of it at the token-type table, where fp16's 2^-11 rounding of the summed streams lands."""
    tap_embs, emb, want = _ref(G, dev, dtype, dropout)
    if full_last:
        monkeypatch.setenv("SIMX_FULL_LAST_LAYER", "1")
    ids, mask, d, dk = _inputs(G, dev)
    enc = _tower(G, dev, dtype, dropout, LAYERS, ckpt)
    assert enc.engine.ccfg.grad_checkpoint == (1 if ckpt else 0)
    fired = []
    if parts > 1:
        enc.engine.grad_ready_hook = lambda e, lo, hi: fired.append((lo, hi))
        enc.engine.bwd_parts = parts
    cls, taps = enc.embed_layers(ids, mask, TAPS)
    assert taps.shape == (len(TAPS), ids.shape[0], emb.shape[1]) and taps.dtype == torch.float32
    (cls * d).sum().add(sum((taps[k] * dk[k]).sum() for k in range(len(TAPS)))).backward()
    got = _grads(enc)
    if parts > 1:
        assert len(fired) == parts and fired[0][1] == enc.engine.n_params and fired[-1][0] == 0
    # ---- forward
    if full_last:                                   # (the other form of the last layer: the bound of the two forms, not bits)
        assert np.abs(cls.detach().cpu().numpy() - emb).max() <= TOL_FWD[dtype] * np.abs(emb).max()
    else:
        assert np.array_equal(cls.detach().cpu().numpy(), emb), "the embedding itself must not change with taps"
    assert torch.equal(taps[-1], cls), "a tap on the last layer is the embedding"
    for k, l in enumerate(TAPS):
        scale = np.abs(tap_embs[k]).max()
        err = np.abs(taps[k].detach().cpu().numpy() - tap_embs[k]).max()
        print("tap %d (%s, p=%.1f): err %.3e of scale %.3e (bound %.1e)" % (l, dtype, dropout, err, scale, TOL_FWD[dtype]))
        assert err <= TOL_FWD[dtype] * scale, "tap on layer %d differs from the %d-layer tower by %.3e (scale %.3e)" % (l, l + 1, err, scale)
    # ---- backward, tensor by tensor
    gscale = max(np.abs(v).max() for v in want.values())
    tol = 2.0 * TWO_FORMS[(dtype, dropout)] + ATOMICS[dtype]
    worst = (0.0, None)
    for name, g in got.items():
        err = np.abs(g - want[name]).max() / gscale
        if err > worst[0]:
            worst = (err, name)
    print("backward (%s, p=%.1f, ckpt=%s, parts=%d, full_last=%s): worst %.3e of the gradient scale at %s (bound %.3e)"
          % (dtype, dropout, ckpt, parts, full_last, worst[0], worst[1], tol))
    assert worst[0] <= tol, "%s off by %.3e of the gradient scale (bound %.3e)" % (worst[1], worst[0], tol)


def test_layers_above_a_tap_get_nothing_from_it(dev, G):
    ids, mask, _, dk = _inputs(G, dev)
    enc = _tower(G, dev, "fp32", 0.0, LAYERS)
    cls, taps = enc.embed_layers(ids, mask, [1])
    (taps[0] * dk[0]).sum().backward()
    got = _grads(enc)
    for name, g in got.items():
        if name.startswith("encoder.layer.2.") or name.startswith("encoder.layer.3."):
            assert not g.any(), name
    assert np.abs(got["encoder.layer.1.output.dense.weight"]).max() > 0 and np.abs(got["encoder.layer.0.attention.self.query.weight"]).max() > 0


def test_taps_without_grad_and_bad_layers(dev, G):
    ids, mask, _, _ = _inputs(G, dev)
    enc = _tower(G, dev, "fp32", 0.0, LAYERS).eval()
    with torch.no_grad():
        cls, taps = enc.embed_layers(ids, mask, [0, 3])
        plain = enc.embed(ids, mask)
    assert torch.equal(cls, plain) and torch.equal(taps[1], plain) and not taps.requires_grad
    for bad in ([3, 0], [4], []):
        with pytest.raises(ValueError):
            enc.embed_layers(ids, mask, bad)
