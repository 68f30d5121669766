"""LEAD/models.py on the MI355X engine: the dual encoder whose forward also returns the [CLS] rows of chosen layers.

The reference's BiBertEncoder (LEAD/models.py:198-242) returns every token of every layer ([n, layers, seq, H]); its
layer-score distillation (LEAD/util.py:609, 635) reads ``[:, layer, 0, :]`` of that and nothing else, so this one returns the
[CLS] rows of the layers it is asked for, [len(layers), n, H], from the encoder's taps (simx_bert_fwd_taps).  Out of scope:
the DistilBERT key schema, ColBERT towers and the add_linear adapters.
"""
from torch import nn

from ..model.models import HFBertEncoder


class BiBertEncoder(nn.Module):
    """LEAD/models.py:198-242.  ``args.pretrained_model_name``: a directory with config.json (+ weights) or a known name;
    ``args.num_hidden_layers`` (optional): the depth of this role's tower (12 for the teacher, 6 for the student of
    distill_from_12de_to_6de.sh), as PROD's student_num_hidden_layers; ``args.share_weight``: one tower for both sides."""

    def __init__(self, args, compute_dtype=None):
        super(BiBertEncoder, self).__init__()
        model_type = str(getattr(args, "model_type", "") or "")
        for kind in ("distilbert", "colbert"):
            if kind in model_type:
                raise NotImplementedError("--model_type %r: %s towers are not on the MI355X path; LEAD's layer-score "
                                          "distillation runs on the BERT tower at any depth" % (model_type, kind))
        if getattr(args, "add_linear", False):
            raise NotImplementedError("--add_linear adapters are not on the MI355X path")
        self.pretrained_model_name = args.pretrained_model_name
        self.model_type = model_type
        mk = lambda: HFBertEncoder.init_encoder(args, model_type=args.pretrained_model_name, compute_dtype=compute_dtype,
                                                num_hidden_layers=getattr(args, "num_hidden_layers", None))
        self.question_model = mk()
        self.ctx_model = self.question_model if getattr(args, "share_weight", False) else mk()

    def query_emb(self, input_ids, attention_mask, layers=None):
        if layers is None:
            return self.question_model.embed(input_ids, attention_mask), None
        return self.question_model.embed_layers(input_ids, attention_mask, layers)

    def body_emb(self, input_ids, attention_mask, layers=None):
        if layers is None:
            return self.ctx_model.embed(input_ids, attention_mask), None
        return self.ctx_model.embed_layers(input_ids, attention_mask, layers)

    def forward(self, query_ids, attention_mask_q, doc_ids=None, attention_mask_d=None, layers=None):
        """-> (q_embs, d_embs, q_layer_cls, d_layer_cls, None): the reference's five positions, with [len(layers), n, H]
        taps (None without ``layers``) where it returns all hidden states."""
        q_embs, q_taps = self.query_emb(query_ids, attention_mask_q, layers)
        d_embs, d_taps = self.body_emb(doc_ids, attention_mask_d, layers)
        return q_embs, d_embs, q_taps, d_taps, None

    def zero_grad(self, set_to_none=False):
        self.question_model.zero_grad()
        self.ctx_model.zero_grad()
