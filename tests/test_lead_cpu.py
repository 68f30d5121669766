"""CPU: the LEAD port's host side -- the closed forms the slot-loss kernels implement (a float64 NumPy restatement held against
the imported reference's autograd, tests/golden/lead_losses.npz), the layer selection, and the rejected flag sets."""
import json
import os
import random
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lead_ref import lead_loss  # noqa: E402

CASES = ("i", "ii", "iii", "iv", "v.r0", "v.r1")


def case_inputs(G, case):
    """(q, ctx, tq, tctx, pos, slots, T, LT, local_q, local_ctx) of a fixture case; the gathered cases v.* share case i's tensors."""
    src = "i" if case.startswith("v.") else case
    loc = lambda k: tuple(int(v) for v in G["%s.%s" % (case, k)]) if case.startswith("v.") else None
    slots = [tuple(float(v) for v in row[:4]) + (int(row[4]),) for row in G[case + ".slots"]]
    return (G[src + ".q"], G[src + ".ctx"], G[src + ".tq"], G[src + ".tctx"], [int(v) for v in G[src + ".pos"]], slots,
            float(G[case + ".T"]), float(G[case + ".LT"]), loc("local_q"), loc("local_ctx"))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "lead_losses.npz"))


def _rel(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() / max(1.0, np.abs(np.asarray(ref)).max())


@pytest.mark.parametrize("case", CASES)
def test_closed_forms_reproduce_reference_autograd(G, case):
    """Without reweighting the restatement is the reference to rounding (1e-11); with it the reference's lambda is a float32
    softmax of float32-rounded inputs, which the restatement follows (f32_lambda) -- 1e-6 is that format's resolution, not a
    property of the closed forms (1.1e-8 absolute was seen against the reference)."""
    q, ctx, tq, tctx, pos, slots, T, LT, lq, lc = case_inputs(G, case)
    out = lead_loss(q, ctx, tq, tctx, pos, slots, T, LT, local_q=lq, local_ctx=lc)
    tol = 1e-6 if any(s[4] for s in slots) else 1e-11
    assert _rel(out["total"], G[case + ".loss"]) <= tol
    assert _rel(out["slot_losses"], G[case + ".slot_losses"]) <= 1e-11
    assert _rel(out["weights"], G[case + ".weights"]) <= tol
    for k in ("dq", "dctx", "dtq", "dtctx"):
        assert out[k].shape == G["%s.%s" % (case, k)].shape
        assert _rel(out[k], G["%s.%s" % (case, k)]) <= tol, k
    n = len(slots) - 1
    d = lambda k: float(G["%s.dict.%s" % (case, k)])
    assert abs(out["slot_losses"][n, 0] - d("loss_db")) <= 1e-11 and abs(out["slot_losses"][n, 2] - d("loss_de_db_dis")) <= 1e-11
    assert abs(out["slot_losses"][n, 3] - d("loss_db_de_dis")) <= 1e-11 and d("loss_db_de_layer_dis") == 0.0
    assert abs(float((out["weights"][:n] * out["slot_losses"][:n, 2]).sum()) - d("loss_de_db_layer_dis")) <= tol


def test_fixture_separates_the_coefficients(G):
    """What makes the fixture discriminating: a wide lambda in case i, lambda = 1 for one layer slot, distinct weights."""
    lam = G["i.weights"][:3]
    assert lam.max() / lam.min() >= 3.0 and abs(lam.sum() - 1.0) < 1e-6
    assert G["iv.weights"][0] == 1.0
    a, b, w, x, _ = G["i.slots"][3]
    assert len({a, b, w, 0.6}) == 4 and w == x and G["iii.slots"][3][1] == 0 and G["iii.slots"][3][3] == 0
    assert float(G["ii.slots"][0][2]) == 0.6 and not G["ii.slots"][:, 4].any()


def test_select_layer_replays_the_reference(golden_dir):
    from simxns_amd.LEAD.util import select_layer
    cases = json.load(open(os.path.join(golden_dir, "lead_select_layer.json")))
    assert len(cases) == 24
    for c in cases:
        a = types.SimpleNamespace(pretrained_model_name=c["pretrained_model_name"], train_file=c["train_file"], add_linear=c["add_linear"],
                                  disitll_layer_num=c["disitll_layer_num"],
                                  **{m: m == c["mode"] for m in ("layer_selection_random", "layer_selection_last", "layer_selection_skip")})
        random.seed(c["seed"])
        got = [select_layer(a) for _ in c["picks"]]
        assert [[list(p[0]), list(p[1])] for p in got] == c["picks"], c


def _loss_args(**kw):
    a = dict(distill_de=True, distill_db=True, distill_de_db_layer_score=True, train_de=True, layer_score_reweight=True, temperature=1.0,
             layer_temperature=10.0, distill_para_db=1.0, distill_para_de=1.0, distill_para_de_db_dis=1.0, distill_para_de_db_layer_score=1.0)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.mark.parametrize("flag", ["distill_col", "distill_ce", "distill_col_db_layer_score", "distill_ce_db_layer_score",
                                  "distill_de_db_attention", "distill_col_db_attention", "distill_ce_db_attention"])
def test_distill_loss_rejects_unsupported_flags(flag):
    """ValueError before any device work: the arguments are not even looked at (None would fail anywhere later)."""
    from simxns_amd.LEAD.util import distill_loss
    with pytest.raises(ValueError, match=flag):
        distill_loss(_loss_args(**{flag: True}), None, None, None, None, None, None, None, None)


@pytest.mark.parametrize("kw", [dict(model_type="distilbert"), dict(model_type="colbert"), dict(model_type="bert", add_linear=True)])
def test_bi_encoder_rejects_unsupported_towers(kw):
    from simxns_amd.LEAD.models import BiBertEncoder
    args = types.SimpleNamespace(pretrained_model_name="/nonexistent", share_weight=True, gradient_checkpointing=False, **kw)
    with pytest.raises(NotImplementedError):
        BiBertEncoder(args)


def test_lead_entry_points_are_declared():
    """The new C-ABI entries are in the header's export list and in the ctypes stub with their argument counts."""
    from simxns_amd import _lib as L
    for name, nargs in (("simx_bert_fwd_taps", 18), ("simx_bert_bwd_taps", 22), ("simx_cls_rows_add_gs", 8),
                        ("simx_lead_scores_workspace_bytes", 7), ("simx_lead_scores_fwd_bwd", 31)):
        assert len(L.SIGNATURES[name][1]) == nargs, name
    hdr = open(os.path.join(ROOT, "include", "simx.h")).read()
    assert "#define SIMX_LEAD_MAX_SLOTS %d" % L.LEAD_MAX_SLOTS in hdr
    import ctypes as C
    assert C.sizeof(L.LeadSlot) == 20


def test_tap_layers_are_validated_on_the_host():
    from simxns_amd.engine import _tap_array
    assert list(_tap_array([0, 2, 3], 4)) == [0, 2, 3]
    for bad in ([], [2, 1], [1, 1], [-1], [4]):
        with pytest.raises(ValueError):
            _tap_array(bad, 4)
