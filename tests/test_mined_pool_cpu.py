"""Host side of the binary mined-negative hand-off (simxns_amd/mined_pool.py, --mined_format / --mined_pool): the pool file
round trip, the positives' CSR, the metrics from first-hit ranks, the flags of the two jobs and of the launcher.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch


def _pool_arrays(nq=5, top=7, seed=0):
    rs = np.random.RandomState(seed)
    pos_cnt = rs.randint(0, 4, size=nq)
    pos_ptr = np.concatenate([[0], np.cumsum(pos_cnt)]).astype(np.int32)
    neg_cnt = rs.randint(0, top + 1, size=nq).astype(np.int32)
    neg_scores = rs.randn(nq, top).astype(np.float32)
    neg_scores[np.arange(top)[None, :] < (top - neg_cnt)[:, None]] = np.inf
    return dict(qids=rs.randint(0, 10 ** 12, size=nq).astype(np.int64), q_tok=rs.randint(0, 30522, size=(nq, 32)).astype(np.int32),
                neg_rows=rs.randint(0, 2 ** 31 - 1, size=(nq, top)).astype(np.int32), neg_scores=neg_scores, neg_cnt=neg_cnt,
                pos_ptr=pos_ptr, pos_rows=rs.randint(0, 1000, size=pos_ptr[-1]).astype(np.int32),
                pos_scores=rs.randn(pos_ptr[-1]).astype(np.float32))


def test_pool_round_trip(tmp_path):
    from simxns_amd import mined_pool as MP
    a = _pool_arrays()
    meta = dict(corpus_rows=1000, q_len=32, p_len=128, pad_id=0, sep_id=102, tokenizer="HashTokenizer", vocab_size=30522, corpus_slices=2)
    path = MP.save_pool(MP.pool_path(str(tmp_path), 6), meta=meta, **a)
    assert os.path.basename(path) == "train_ce_6.pool.npz" and not os.path.exists(path + ".tmp")
    b = MP.load_pool(path)
    for k in MP.POOL_FIELDS:
        assert b[k].dtype == a[k].dtype and b[k].shape == a[k].shape and b[k].tobytes() == a[k].tobytes(), k
    assert b["meta"] == dict(meta, version=MP.FORMAT_VERSION, top=7, nq=5)
    # scores are widened exactly: float32 -> float64 -> float32 keeps the bits (+inf padding included)
    assert np.array_equal(b["neg_scores"].astype(np.float64).astype(np.float32).view(np.uint32), a["neg_scores"].view(np.uint32))
    # uncompressed: the file is at least as large as the arrays
    assert os.path.getsize(path) >= sum(v.nbytes for v in a.values())
    with pytest.raises(ValueError):
        MP.save_pool(str(tmp_path / "bad.pool.npz"), meta=meta, **dict(a, neg_cnt=a["neg_cnt"][:-1]))
    other = dict(np.load(path))
    other["meta"] = np.array(json.dumps(dict(b["meta"], version=MP.FORMAT_VERSION + 1)))
    np.savez(str(tmp_path / "future.npz"), **other)
    with pytest.raises(ValueError, match="version"):
        MP.load_pool(str(tmp_path / "future.npz"))


def test_positives_csr_order_dedup_and_missing_pid():
    from simxns_amd.mined_pool import positives_csr
    passage_ids = np.array([50, 10, 40, 30, 20, 70], np.int64)            # pid -> corpus row is no identity and not sorted
    qids = np.array([7, 8, 9, 11], np.int64)
    pos_qp = {7: [30, 10], 8: [70], 11: [20, 20]}
    pos_add = {7: [10, 50, 30], 9: [40], 12: [99]}                       # repeats a qrels positive; a query only in the additions
    ptr, rows = positives_csr(qids, pos_qp, pos_add, passage_ids)
    assert ptr.dtype == np.int32 and rows.dtype == np.int64
    assert ptr.tolist() == [0, 3, 4, 5, 6]
    assert rows.tolist() == [3, 1, 0, 5, 2, 4]                           # pids 30, 10, 50 | 70 | 40 | 20: first-occurrence order
    # the key order of write_to_file's temp_pos
    for i, q in enumerate(qids):
        keys = list({e: 0 for e in pos_qp.get(int(q), []) + pos_add.get(int(q), [])})
        assert [int(passage_ids[r]) for r in rows[ptr[i]:ptr[i + 1]]] == keys
    ptr0, rows0 = positives_csr(qids, {}, {}, passage_ids)
    assert ptr0.tolist() == [0] * 5 and rows0.shape == (0,)
    with pytest.raises(ValueError, match=r"passage 99 of query 9 "):
        positives_csr(qids, pos_qp, {9: [40, 99]}, passage_ids)
    with pytest.raises(ValueError, match=r"passage 5 of query 7 "):       # below every pid of the corpus
        positives_csr(qids, {7: [5]}, {}, passage_ids)


def test_metrics_from_first_hit_equals_compute_metrics():
    from simxns_amd.co_training.co_training_generate import compute_metrics
    from simxns_amd.mined_pool import metrics_from_first_hit
    # first relevant rank per query (1-based, 0 = never): the boundaries of MRR@10 and recall@50, an unlabelled query, a labelled
    # query that was not ranked
    hits = [1, 2, 10, 11, 50, 51, 0, 3, 7]
    qids = list(range(100, 100 + len(hits)))
    gold = {q: [1000 + q] for q in qids if q != 107}                      # 107 has no labels
    gold[999] = [5]                                                       # labelled, not ranked: counts in the denominator
    cand = {}
    for q, h in zip(qids, hits):
        c = list(range(60))
        if h:
            c[h - 1] = 1000 + q
        cand[q] = c
    want = compute_metrics(gold, cand)
    got = metrics_from_first_hit(np.array(hits, np.int32), np.array([q in gold for q in qids]), len(gold))
    assert got == want and list(got) == list(want)
    assert got["recall@1"] == 1 / 9 and got["recall@50"] == 6 / 9 and got["recall@all"] == 7 / 9 and got["QueriesRanked"] == 9
    with pytest.raises(IOError):
        metrics_from_first_hit(np.array([1, 0]), np.array([False, False]), 3)
    with pytest.raises(IOError):
        compute_metrics({1: [2]}, {5: [2]})


def test_corpus_token_slices_reuse_and_gather(tmp_path):
    from simxns_amd import mined_pool as MP
    from simxns_amd.utils.MARCO_until_new import HashTokenizer
    tok, d = HashTokenizer(), str(tmp_path)
    table = np.arange(11 * 8, dtype=np.int32).reshape(11, 8)
    desc = MP.corpus_tok_description(11, 8, tok, 3)
    assert desc == dict(tokenizer="HashTokenizer", vocab_size=30522, rows=11, p_len=8, world=3)
    assert MP.load_corpus_slice(d, 0, 3, desc) is None                    # nothing there yet
    for r in range(3):
        lo, hi = MP.corpus_slice(r, 3, 11)
        assert os.path.basename(MP.save_corpus_slice(d, r, 3, table[lo:hi])) == "corpus_tok.r%dof3.npy" % r
    assert MP.load_corpus_slice(d, 1, 3, desc) is None                    # slices without their description are not trusted
    MP.write_corpus_tok_description(d, desc)
    lo, hi = MP.corpus_slice(1, 3, 11)
    assert np.array_equal(MP.load_corpus_slice(d, 1, 3, desc), table[lo:hi])
    assert MP.load_corpus_slice(d, 1, 3, dict(desc, p_len=16)) is None    # another description: rewritten, not reused
    meta = dict(tokenizer="HashTokenizer", vocab_size=30522, p_len=8, corpus_rows=11, corpus_slices=3)
    rows = np.array([0, 2, 3, 4, 9, 10])
    assert np.array_equal(MP.gather_corpus_rows(d, rows, meta), table[rows])
    assert MP.gather_corpus_rows(d, np.zeros(0, np.int64), meta).shape == (0, 8)
    with pytest.raises(ValueError, match="mined with"):
        MP.gather_corpus_rows(d, rows, dict(meta, vocab_size=100))
    with pytest.raises(ValueError):
        MP.gather_corpus_rows(d, np.array([3, 11]), meta)


def test_dataset_from_pool_shards_and_refuses_text_access(tmp_path):
    from simxns_amd import mined_pool as MP
    from simxns_amd.utils.MARCO_until_new import HashTokenizer, Rocketqa_v2Dataset
    a = _pool_arrays(nq=7)
    meta = dict(corpus_rows=1000, q_len=32, p_len=128, pad_id=0, sep_id=102, tokenizer="HashTokenizer", vocab_size=30522, corpus_slices=1)
    path = MP.save_pool(MP.pool_path(str(tmp_path), 6), meta=meta, **a)
    sizes = []
    for rank in range(3):
        ds = Rocketqa_v2Dataset(str(tmp_path / "train_ce_6.tsv"), HashTokenizer(), num_hard_negatives=1, trainer_id=rank, trainer_num=3,
                                corpus_path=str(tmp_path), pool_path=path)     # neither the .tsv nor para.txt exists: nothing reads them
        assert ds.mined_rows.tolist() == list(range(rank, 7, 3))
        sizes.append(len(ds))
        with pytest.raises(RuntimeError, match="no text"):
            ds[0]
    assert sizes == [3, 2, 2]


def test_train_job_refuses_mined_pool_with_the_host_sampler(capsys):
    from simxns_amd.co_training import co_training_marco_train as T
    for argv in (["--mined_pool"], ["--mined_pool", "--sampler", "host"]):
        with pytest.raises(SystemExit):
            T.get_arguments(argv)
        assert "--mined_pool needs --sampler gpu" in capsys.readouterr().err
    args = T.get_arguments(["--mined_pool", "--sampler", "gpu"])
    assert args.mined_pool is True
    assert T.get_arguments([]).mined_pool is False


def test_generate_job_mined_format_flag():
    from simxns_amd.co_training import co_training_generate as Gn
    base = ["--model_type", "m", "--output_dir", "o", "--passage_path", "p"]
    assert Gn.get_arguments(base).mined_format == "tsv"
    assert [Gn.get_arguments(base + ["--mined_format", f]).mined_format for f in Gn.MINED_FORMATS] == ["tsv", "pool", "both"]
    with pytest.raises(SystemExit):
        Gn.get_arguments(base + ["--mined_format", "json"])


def test_launcher_mined_pool(capsys, golden_dir):
    from simxns_amd import launch
    from simxns_amd.co_training import co_training_generate as Gn
    from simxns_amd.co_training import co_training_marco_train as T
    # without the flag: the command lines of the parent commit, to the letter
    launch.main(["MS_Pas", "--dry-run", "--nproc", "8", "--last-step", "5000"])
    out = capsys.readouterr().out
    assert out.replace(sys.executable, "PYTHON") == open(os.path.join(golden_dir, "launch_ms_pas_dry_run.txt")).read()
    assert "mined" not in out
    launch.main(["MS_Pas", "--dry-run", "--nproc", "8", "--last-step", "0", "--mined_pool"])
    train, gen = capsys.readouterr().out.splitlines()
    assert "co_training_marco_train.py" in train and "--mined_pool" in train.split() and "--sampler=gpu" in train.split()
    assert "co_training_generate.py" in gen and "--mined_format=pool" in gen.split() and "--mined_pool" not in gen.split()
    # and the two jobs parse them
    assert T.get_arguments(train.split()[train.split().index("simxns_amd/co_training/co_training_marco_train.py") + 1:]).mined_pool is True
    assert Gn.get_arguments(gen.split()[gen.split().index("simxns_amd/co_training/co_training_generate.py") + 1:]).mined_format == "pool"
    for recipe in ("NQ", "TQ", "MS_Doc"):
        with pytest.raises(SystemExit):
            launch.main([recipe, "--dry-run", "--mined_pool"])
        assert "--mined_pool is for the MS_Pas recipe only" in capsys.readouterr().err


def test_mine_negatives_refuses_cpu_tensors():
    from simxns_amd import _lib as L
    from simxns_amd import ops
    D, I = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(L.SimxError, match="HIP device"):
        ops.mine_negatives(D, I, torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int64))
    assert "simx_mine_negatives" in L.SIGNATURES and hasattr(L.load(), "simx_mine_negatives")
