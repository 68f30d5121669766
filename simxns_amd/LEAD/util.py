"""LEAD/util.py on the MI355X engine: layer selection and the distillation loss of the 12de -> 6de recipe.

distill_loss covers the flag set of LEAD/distillation/distill_from_12de_to_6de.sh -- distill_de + distill_db with
distill_de_db_layer_score, with or without train_de / layer_score_reweight -- as ONE call of ops.lead_layer_score_loss
(simx_lead_scores_fwd_bwd): no per-layer launch sequence and no device -> host read (the reference's
``torch.tensor([...])`` of the per-layer teacher losses is one synchronisation per layer).  The ColBERT / cross-encoder
teachers and the attention-map (VIRT) terms are out of scope and rejected before any device work.
"""
from random import sample

import torch

from .. import ops

UNSUPPORTED_FLAGS = ("distill_col", "distill_ce", "distill_col_db_layer_score", "distill_ce_db_layer_score",
                     "distill_de_db_attention", "distill_col_db_attention", "distill_ce_db_attention")


def select_layer(args):
    """LEAD/util.py:206-254, literally (same random.sample calls in the same order): the student's and the teacher's layer
    indices, sorted, so that the i-th student layer is paired with the i-th teacher layer."""
    selected_index_list_db, selected_index_list_teacher = None, None
    if args.layer_selection_random:
        if 'large' not in args.pretrained_model_name:
            all_layer_index = [i for i in range(7 if args.add_linear else 6)]
            selected_index_list_db = sorted(sample(all_layer_index, args.disitll_layer_num))
            all_layer_index = [i for i in range(13 if args.add_linear else 12)]
            selected_index_list_teacher = sorted(sample(all_layer_index, args.disitll_layer_num))
        else:
            all_layer_index = [i for i in range(13 if args.add_linear else 12)]
            selected_index_list_db = sorted(sample(all_layer_index, args.disitll_layer_num))
            all_layer_index = [i for i in range(25 if args.add_linear else 24)]
            selected_index_list_teacher = sorted(sample(all_layer_index, args.disitll_layer_num))
    elif args.layer_selection_last:
        # pas distill 5 layers, doc distill 6 layers
        if 'ms' in args.train_file:
            selected_index_list_db = [1, 2, 3, 4, 5]
            selected_index_list_teacher = [7, 8, 9, 10, 11]
        else:
            selected_index_list_db = [0, 1, 2, 3, 4, 5]
            selected_index_list_teacher = [6, 7, 8, 9, 10, 11]
    elif args.layer_selection_skip:
        if 'ms' in args.train_file:
            selected_index_list_db = [1, 2, 3, 4, 5]
            selected_index_list_teacher = [0, 2, 4, 6, 8]
        else:
            selected_index_list_db = [0, 1, 2, 3, 4, 5]
            selected_index_list_teacher = [0, 2, 4, 6, 8, 10]
    return selected_index_list_db, selected_index_list_teacher


def check_flags(args):
    """The objectives this port has: raises ValueError for every other one, before anything touches a device."""
    bad = [f for f in UNSUPPORTED_FLAGS if getattr(args, f, False)]
    if bad:
        raise ValueError("LEAD flags %s: the ColBERT / cross-encoder teachers and the attention-map terms are not on the MI355X "
                         "path (distill_de + distill_db + distill_de_db_layer_score is)" % ", ".join("--" + f for f in bad))
    if not (getattr(args, "distill_de", False) and getattr(args, "distill_db", False)):
        raise ValueError("LEAD distill_loss needs --distill_de and --distill_db (the 12de -> 6de recipe)")


def slot_weights(args, n_layers):
    """(a, b, w, x, reweight) per slot -- the layer slots, then the final slot of the pooled embeddings (LEAD/util.py:737-764)."""
    train_de = bool(getattr(args, "train_de", False))
    rw = bool(getattr(args, "layer_score_reweight", False))
    layer = (0.0, 0.0, 0.0 if rw else float(args.distill_para_de_db_layer_score), 0.0, rw)
    dis = float(args.distill_para_de_db_dis)
    final = (float(args.distill_para_db), float(args.distill_para_de) if train_de else 0.0, dis, dis if train_de else 0.0, False)
    return [layer] * n_layers + [final]


def distill_loss(args, q_embs_dual, q_embs_db, d_embs_dual, d_embs_db, q_layer_cls_dual, d_layer_cls_dual, q_layer_cls_db,
                 d_layer_cls_db, loss_scale=None, local_q=None, local_ctx=None):
    """LEAD/util.py:561-831 for distill_de + distill_db (+ distill_de_db_layer_score): *_dual the teacher's, *_db the student's
    pooled embeddings [Q|C, H] and tapped [CLS] rows [n, Q|C, H] (already the selected layers, paired by position; None
    without distill_de_db_layer_score).  -> (loss, loss_dict) with the reference's keys; the dict entries are detached
    device scalars.  local_q / local_ctx: the rows of a gathered batch that carry gradient, as in ops.inbatch_nll_loss."""
    check_flags(args)
    layer_score = bool(getattr(args, "distill_de_db_layer_score", False)) and q_layer_cls_db is not None
    n = q_layer_cls_db.shape[0] if layer_score else 0
    if layer_score:
        q = torch.cat([q_layer_cls_db, q_embs_db.unsqueeze(0)], 0)
        c = torch.cat([d_layer_cls_db, d_embs_db.unsqueeze(0)], 0)
        tq = torch.cat([q_layer_cls_dual, q_embs_dual.unsqueeze(0)], 0)
        tc = torch.cat([d_layer_cls_dual, d_embs_dual.unsqueeze(0)], 0)
    else:
        q, c, tq, tc = (t.unsqueeze(0) for t in (q_embs_db, d_embs_db, q_embs_dual, d_embs_dual))
    Q, C = q.shape[1], c.shape[1]
    sample_num = C // Q
    target = [i * sample_num for i in range(Q)]
    train_de = bool(getattr(args, "train_de", False))
    loss, sl, w = ops.lead_layer_score_loss(q, c, tq, tc, target, slot_weights(args, n), args.temperature,
                                            getattr(args, "layer_temperature", 1.0), teacher_grad=train_de,
                                            loss_scale=loss_scale, local_q=local_q, local_ctx=local_ctx)
    loss_dict = {'loss_db': sl[n, 0]}
    if train_de:
        loss_dict['loss_dual'] = sl[n, 1]
    loss_dict['loss_de_db_dis'], loss_dict['loss_db_de_dis'] = sl[n, 2], sl[n, 3]
    if layer_score:
        for i in range(n):
            loss_dict['loss_score_layer_dis_%d' % i] = sl[i, 2]
        loss_dict['loss_de_db_layer_dis'] = (w[:n] * sl[:n, 2]).sum()
        loss_dict['loss_db_de_layer_dis'] = 0          # (the reference never assigns it: LEAD/util.py:552-559)
    return loss, loss_dict
