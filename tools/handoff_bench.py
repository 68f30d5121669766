"""Hand-off of the mined hard negatives from the generate job to the train job on one GPU (not part of bench.py's metric): from
"search result D, I [nq,k] on the device" to "the train job's device pool ready", by the two paths of the MS-Pas recipe on the same
synthetic result, one JSON record:

  text  D, I -> host, the two dictionary comprehensions of RenewTools.get_question_topk, write_to_file (train_ce_<step>.tsv),
        Rocketqa_v2Dataset (read_sharded_tsv) and its build_device_pool (parse, right-aligned tables, upload)
  pool  positives_csr, ops.mine_negatives on the device, save_pool (train_ce_<step>.pool.npz), Rocketqa_v2Dataset(pool_path=...)
        and its build_device_pool (load_pool, tables, passage tokens gathered from the corpus-token slices, upload)

No model and no reference.  PASSAGE TOKENISING IS EXCLUDED FROM BOTH: the text path's dataset gets a tokenizer whose encode returns a
constant three-token list (what stays is the call, the padding and the list -> array conversion of build_device_pool), and the pool
path reads a synthetic int32 token table saved beforehand, outside the timed part, the way the generate job saves its slices.
The text path is bound by the host's speed; the record holds both times as measured and no target ratio.
usage: python tools/handoff_bench.py [--nq 20000] [--k 200] [--corpus_rows 200000] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from simxns_amd import mined_pool as MP                                                   # noqa: E402
from simxns_amd import ops                                                                # noqa: E402
from simxns_amd.co_training.co_training_generate import write_to_file                    # noqa: E402
from simxns_amd.utils.MARCO_until_new import HashTokenizer, Rocketqa_v2Dataset            # noqa: E402


class _ConstantTokenizer(HashTokenizer):
    def encode(self, text, text_pair=None, **kw):
        return [self.cls_token_id, 2000, self.sep_token_id]


class _NoTextDataset(Rocketqa_v2Dataset):
    def _encode_ctx(self, pid):
        return [101, 2000, 102]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=20000)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--corpus_rows", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, k, rows, top, N = a.nq, a.k, a.corpus_rows, 200, 15
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    # a search result with distinct ids per row: id = (base + rank * step) mod rows, step coprime to rows
    step = rs.randint(1, rows, size=nq).astype(np.int64)
    while True:
        bad = np.gcd(step, rows) != 1
        if not bad.any():
            break
        step[bad] = rs.randint(1, rows, size=int(bad.sum()))
    base = rs.randint(0, rows, size=nq).astype(np.int64)
    I_host = (base[:, None] + np.arange(k, dtype=np.int64)[None, :] * step[:, None]) % rows
    D_host = np.sort((rs.randn(nq, k) * 3 + 70).astype(np.float32), axis=1)[:, ::-1].copy()
    # one positive per query at "rank" 0..299 of the same progression: about two thirds are among the k retrieved
    pos_rank = rs.randint(0, 300, size=nq)
    pos_row = (base + pos_rank * step) % rows
    qids = np.arange(nq, dtype=np.int64) * 3 + 1
    passage_ids = np.arange(rows, dtype=np.int64)
    pos_qp = {int(q): [int(p)] for q, p in zip(qids, pos_row)}
    questions = [[int(q), "synthetic query %d" % q] for q in qids]
    tok = HashTokenizer()
    qtab = np.zeros((nq, 32), np.int32)
    qtab[:, :3] = [101, 2000, 102]
    D, I = torch.from_numpy(D_host).to(dev), torch.from_numpy(I_host).to(dev)
    rec = dict(nq=nq, k=k, top=top, corpus_rows=rows, number_neg=N, device=torch.cuda.get_device_name(0),
               tokenising="excluded from both paths (see the tool's docstring)")
    with tempfile.TemporaryDirectory() as d:
        # outside the timed part: the corpus-token slice the generate job keeps in --ann_dir, and a warm-up launch
        MP.save_corpus_slice(d, 0, 1, rs.randint(0, 30522, size=(rows, 128)).astype(np.int32))
        MP.write_corpus_tok_description(d, MP.corpus_tok_description(rows, 128, tok, 1))
        ptr0, rows0 = MP.positives_csr(qids[:8], pos_qp, {}, passage_ids)
        ops.mine_negatives(D[:8], I[:8], torch.from_numpy(ptr0).to(dev), torch.from_numpy(rows0).to(dev), top=top)
        torch.cuda.synchronize()

        # ---- text path
        t = [time.perf_counter()]
        Dh, Ih = D.cpu().numpy(), I.cpu().numpy()
        cand = {int(q): [int(passage_ids[j]) for j in Ih[r] if j >= 0] for r, q in enumerate(qids)}
        scores = {int(q): [float(s) for s, j in zip(Dh[r], Ih[r]) if j >= 0] for r, q in enumerate(qids)}
        t.append(time.perf_counter())
        tsv = write_to_file(cand, scores, questions, pos_qp, {}, "train", d, 1)
        t.append(time.perf_counter())
        text = _NoTextDataset(tsv, _ConstantTokenizer(), num_hard_negatives=N, p_text={}, p_title={})
        P = text.build_device_pool(dev)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        rec["text"] = dict(seconds=round(t[3] - t[0], 4), dicts_s=round(t[1] - t[0], 4), write_s=round(t[2] - t[1], 4),
                           read_parse_tables_upload_s=round(t[3] - t[2], 4), file_mb=round(os.path.getsize(tsv) / 1e6, 1))

        # ---- pool path
        t = [time.perf_counter()]
        ptr, prow = MP.positives_csr(qids, pos_qp, {}, passage_ids)
        out = ops.mine_negatives(D, I, torch.from_numpy(ptr).to(dev), torch.from_numpy(prow).to(dev), top=top)
        host = {n: v.cpu().numpy() for n, v in out.items()}
        t.append(time.perf_counter())
        meta = dict(MP.tokenizer_description(tok), corpus_rows=rows, q_len=32, p_len=128, pad_id=0, sep_id=102, corpus_slices=1, step=1)
        path = MP.save_pool(MP.pool_path(d, 1), qids, qtab, host["neg_rows"], host["neg_scores"], host["neg_cnt"], ptr, prow, host["pos_scores"], meta)
        t.append(time.perf_counter())
        binary = Rocketqa_v2Dataset(tsv, tok, num_hard_negatives=N, pool_path=path)
        B = binary.build_device_pool(dev)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        rec["pool"] = dict(seconds=round(t[3] - t[0], 4), csr_mine_copy_s=round(t[1] - t[0], 4), save_s=round(t[2] - t[1], 4),
                           load_tables_gather_upload_s=round(t[3] - t[2], 4), file_mb=round(os.path.getsize(path) / 1e6, 1))
        rec["pools_equal"] = bool(all(torch.equal(P[n], B[n]) for n in ("cand_scores", "pos_scores", "pos_cnt")))
        rec["passages_in_pool"] = int(B["p_tok"].shape[0])
    rec["text_over_pool"] = round(rec["text"]["seconds"] / rec["pool"]["seconds"], 1)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if rec["pools_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
