"""The training step of LEAD/run_LEAD.py (lines 156-227) for the 12de -> 6de layer-score recipe on the MI355X engine.

The data set classes, the command-line loop and evaluation are not ported: the caller owns the loop,
zeroes the gradients and steps the optimisers (simxns_amd.optim), as with ProD_KD's step.
"""
import torch

from .util import check_flags, distill_loss


def lead_distill_step(args, model_de, model_db, batch_retriever, selected_db, selected_teacher, loss_scale=None):
    """One micro-step: the two forwards with [CLS] taps on the selected layers, the distillation loss,
    ``loss / gradient_accumulation_steps`` and its backward into both towers' gradient buffers (the teacher's only with
    ``args.train_de``).  batch_retriever = (query_ids, attention_mask_q, doc_ids, attention_mask_d, ...) as the reference's
    collate yields it.  -> (loss, loss_dict), detached."""
    check_flags(args)
    dev = next(model_db.parameters()).device
    q_ids, q_mask, d_ids, d_mask = (t.long().to(dev) for t in batch_retriever[:4])
    taps = bool(getattr(args, "distill_de_db_layer_score", False))
    model_db.train()
    q_db, d_db, q_l_db, d_l_db, _ = model_db(q_ids, q_mask, d_ids, d_mask, layers=list(selected_db) if taps else None)
    train_de = bool(getattr(args, "train_de", False))
    model_de.train(train_de)
    with torch.set_grad_enabled(train_de):
        q_de, d_de, q_l_de, d_l_de, _ = model_de(q_ids, q_mask, d_ids, d_mask, layers=list(selected_teacher) if taps else None)
    loss, loss_dict = distill_loss(args, q_de, q_db, d_de, d_db, q_l_de, d_l_de, q_l_db, d_l_db, loss_scale=loss_scale)
    loss = loss / args.gradient_accumulation_steps
    loss.backward()
    return loss.detach(), loss_dict
