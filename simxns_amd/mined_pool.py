"""Binary hand-off of the mined hard negatives from the MS-Pas generate job to the train job's device sampler
(``--mined_format pool`` / ``--mined_pool``): what ``write_to_file`` formats as text and ``Rocketqa_v2Dataset.build_device_pool``
parses back, kept as the arrays ``ops.mine_negatives`` produced on the device.

  train_ce_<step>.pool.npz   one uncompressed .npz per iteration (``save_pool`` / ``load_pool``):
      qids int64 [nq], q_tok int32 [nq, q_len], neg_rows int32 [nq, top], neg_scores float32 [nq, top] (right-aligned behind
      (row 0, +inf) padding), neg_cnt int32 [nq], pos_ptr int32 [nq+1], pos_rows int32, pos_scores float32 (CSR, the order of
      write_to_file's positive column) and ``meta`` (JSON).  Rows are CORPUS ROWS (line numbers of para.txt), not pids.
  corpus_tok.r<rank>of<world>.npy + corpus_tok.json   the int32 token table of every generate rank's contiguous corpus slice,
      written once per --ann_dir and reused while the description in the json matches.

Everything here is host NumPy over whole arrays; nothing loops over (query, candidate) pairs.
"""
import json
import os

import numpy as np

FORMAT_VERSION = 1
POOL_FIELDS = ("qids", "q_tok", "neg_rows", "neg_scores", "neg_cnt", "pos_ptr", "pos_rows", "pos_scores")
_DTYPES = dict(qids=np.int64, q_tok=np.int32, neg_rows=np.int32, neg_scores=np.float32, neg_cnt=np.int32, pos_ptr=np.int32,
               pos_rows=np.int32, pos_scores=np.float32)


def pool_path(ann_dir, step, mode="train"):
    return os.path.join(ann_dir, "%s_ce_%s.pool.npz" % (mode, step))


def tokenizer_description(tokenizer):
    return {"tokenizer": type(tokenizer).__name__, "vocab_size": int(getattr(tokenizer, "vocab_size", 0) or 0)}


def positives_csr(qids, pos_qp, pos_qp_add, passage_ids):
    """-> (pos_ptr int32 [nq+1], pos_rows int64): per query the pids ``pos_qp[q] + pos_qp_add[q]`` deduplicated in
    first-occurrence order (the key order of write_to_file's ``temp_pos``), mapped to corpus rows by one vectorised inverse of
    ``passage_ids``.  A positive pid that is not in the corpus raises ValueError naming it."""
    per_query = [list(dict.fromkeys(pos_qp.get(int(q), []) + pos_qp_add.get(int(q), []))) for q in qids]
    pos_ptr = np.zeros(len(per_query) + 1, np.int64)
    np.cumsum([len(p) for p in per_query], out=pos_ptr[1:])
    if pos_ptr[-1] > np.iinfo(np.int32).max:
        raise ValueError("positives_csr: %d positives do not fit the int32 offsets" % pos_ptr[-1])
    pids = np.fromiter((p for ps in per_query for p in ps), np.int64, int(pos_ptr[-1]))
    passage_ids = np.asarray(passage_ids, np.int64)
    order = np.argsort(passage_ids, kind="stable")
    at = np.searchsorted(passage_ids, pids, sorter=order)
    rows = order[np.minimum(at, len(order) - 1)] if len(order) else np.zeros(len(pids), np.int64)
    missing = (passage_ids[rows] != pids) if len(order) else np.ones(len(pids), bool)
    if missing.any():
        slot = int(np.flatnonzero(missing)[0])
        q = int(np.searchsorted(pos_ptr, slot, side="right")) - 1
        raise ValueError("positive passage %d of query %d is not in the corpus" % (int(pids[slot]), int(qids[q])))
    return pos_ptr.astype(np.int32), rows.astype(np.int64)


def metrics_from_first_hit(first_hit, labelled, n_labelled):
    """The dictionary of co_training_generate.compute_metrics from ``first_hit`` [nq] (1 + rank of the first relevant passage,
    0 = none; ops.mine_negatives against the qrels positives) and ``labelled`` [nq] (the query has relevance labels):
    same keys, same denominators (n_labelled = the number of labelled queries), same IOError when no ranked query is labelled."""
    first_hit = np.asarray(first_hit).astype(np.int64)
    labelled = np.asarray(labelled, bool)
    if not labelled.any():
        raise IOError("No matching QIDs found. Are you sure you are scoring the evaluation set?")
    fh = first_hit[labelled]
    mrr = 0.0
    for r in fh[(fh >= 1) & (fh <= 10)].tolist():              # in query order: the sum compute_metrics accumulates
        mrr += 1.0 / r
    n = int(n_labelled)
    return {"MRR @10": mrr / n, "recall@1": int((fh == 1).sum()) / n, "recall@50": int(((fh >= 1) & (fh <= 50)).sum()) / n,
            "recall@all": int((fh >= 1).sum()) / n, "QueriesRanked": int(first_hit.shape[0])}


def save_pool(path, qids, q_tok, neg_rows, neg_scores, neg_cnt, pos_ptr, pos_rows, pos_scores, meta):
    """One uncompressed .npz (written beside ``path`` and renamed into place).  ``meta``: a dict; ``version``, ``top``, ``nq`` are
    filled in here."""
    arrays = dict(qids=qids, q_tok=q_tok, neg_rows=neg_rows, neg_scores=neg_scores, neg_cnt=neg_cnt, pos_ptr=pos_ptr,
                  pos_rows=pos_rows, pos_scores=pos_scores)
    arrays = {k: np.ascontiguousarray(np.asarray(v), dtype=_DTYPES[k]) for k, v in arrays.items()}
    nq = arrays["qids"].shape[0]
    if not (arrays["q_tok"].ndim == 2 and arrays["q_tok"].shape[0] == nq and arrays["neg_rows"].ndim == 2
            and arrays["neg_rows"].shape == arrays["neg_scores"].shape and arrays["neg_rows"].shape[0] == nq
            and arrays["neg_cnt"].shape == (nq,) and arrays["pos_ptr"].shape == (nq + 1,)
            and arrays["pos_rows"].shape == arrays["pos_scores"].shape == (int(arrays["pos_ptr"][-1]),)):
        raise ValueError("save_pool: inconsistent shapes %s" % {k: v.shape for k, v in arrays.items()})
    meta = dict(meta, version=FORMAT_VERSION, top=int(arrays["neg_rows"].shape[1]), nq=int(nq))
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        np.savez(f, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    os.replace(tmp, path)
    return path


def load_pool(path):
    """-> dict of the arrays of ``save_pool`` (their stored dtypes) + ``meta`` (dict)."""
    with np.load(path, allow_pickle=False) as z:
        out = {k: z[k] for k in POOL_FIELDS}
        out["meta"] = json.loads(str(z["meta"][()]))
    if out["meta"].get("version") != FORMAT_VERSION:
        raise ValueError("%s: pool format version %r, this build reads %d" % (path, out["meta"].get("version"), FORMAT_VERSION))
    for k in POOL_FIELDS:
        if out[k].dtype != _DTYPES[k]:
            raise ValueError("%s: %s is %s, expected %s" % (path, k, out[k].dtype, np.dtype(_DTYPES[k])))
    return out


# ---- corpus token table: one slice per generate rank ---------------------------------------------------------------------------------
def corpus_slice(rank, world, rows):
    return rank * rows // world, (rank + 1) * rows // world


def corpus_tok_paths(ann_dir, rank, world):
    return os.path.join(ann_dir, "corpus_tok.r%dof%d.npy" % (rank, world)), os.path.join(ann_dir, "corpus_tok.json")


def corpus_tok_description(rows, p_len, tokenizer, world):
    return dict(tokenizer_description(tokenizer), rows=int(rows), p_len=int(p_len), world=int(world))


def read_corpus_tok_description(ann_dir):
    path = corpus_tok_paths(ann_dir, 0, 1)[1]
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def load_corpus_slice(ann_dir, rank, world, description):
    """This rank's saved slice (memory-mapped) when corpus_tok.json matches ``description`` and the slice has its shape, else None."""
    if read_corpus_tok_description(ann_dir) != description:
        return None
    path = corpus_tok_paths(ann_dir, rank, world)[0]
    if not os.path.exists(path):
        return None
    tab = np.load(path, mmap_mode="r")
    lo, hi = corpus_slice(rank, world, description["rows"])
    if tab.dtype != np.int32 or tab.shape != (hi - lo, description["p_len"]):
        return None
    return tab


def save_corpus_slice(ann_dir, rank, world, table):
    path = corpus_tok_paths(ann_dir, rank, world)[0]
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        np.save(f, np.ascontiguousarray(table, dtype=np.int32))
    os.replace(tmp, path)
    return path


def write_corpus_tok_description(ann_dir, description):
    """Written by ONE rank, after every rank has compared the old description with its own (the generate job: after the merged search)."""
    path = corpus_tok_paths(ann_dir, 0, 1)[1]
    if read_corpus_tok_description(ann_dir) == description:
        return path
    with open(path + ".tmp", "w") as f:
        json.dump(description, f, indent=2, sort_keys=True)
    os.replace(path + ".tmp", path)
    return path


def gather_corpus_rows(ann_dir, rows, meta):
    """int32 [len(rows), p_len]: the token rows of the ascending corpus rows ``rows`` from the memory-mapped slices; the description
    beside them must be the one the pool was mined with (``meta``)."""
    desc = read_corpus_tok_description(ann_dir)
    want = {k: meta[k] for k in ("tokenizer", "vocab_size", "p_len")}
    want.update(rows=meta["corpus_rows"], world=meta["corpus_slices"])
    if desc != want:
        raise ValueError("corpus token slices in %s are %s, the pool was mined with %s" % (ann_dir, desc, want))
    rows = np.asarray(rows, np.int64)
    out = np.empty((len(rows), desc["p_len"]), np.int32)
    if len(rows) and (rows[0] < 0 or rows[-1] >= desc["rows"] or (np.diff(rows) < 0).any()):
        raise ValueError("gather_corpus_rows: rows must ascend inside [0, %d)" % desc["rows"])
    for r in range(desc["world"]):
        lo, hi = corpus_slice(r, desc["world"], desc["rows"])
        a, b = np.searchsorted(rows, [lo, hi])
        if b > a:
            tab = np.load(corpus_tok_paths(ann_dir, r, desc["world"])[0], mmap_mode="r")
            if tab.dtype != np.int32 or tab.shape != (hi - lo, desc["p_len"]):
                raise ValueError("corpus token slice %d of %d in %s has shape %s, expected %s" % (r, desc["world"], ann_dir, tab.shape,
                                                                                                   (hi - lo, desc["p_len"])))
            out[a:b] = tab[rows[a:b] - lo]
    return out
