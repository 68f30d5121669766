"""Device-side hand-off of the mined hard negatives (ops.mine_negatives -> train_ce_<step>.pool.npz -> the train job's device pool)
against the repository's own text path: co_training_generate.write_to_file, then the parse Rocketqa_v2Dataset.build_device_pool does
(read_sharded_tsv + parse_pairs).  Everything is compared for exact equality, scores as float32 bits."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCORPUS = 5000
SHAPES = [(1, 1), (63, 200), (64, 64), (65, 200), (200, 200), (1000, 200)]
CASES = ("none", "rank0", "last", "beyond_top", "never", "seventy", "all_positive", "five_valid", "ties", "rank11", "rank51")


def _pid(rows):
    """corpus row -> pid of the synthetic corpus (no identity, so a row mistaken for a pid shows)"""
    return np.asarray(rows, np.int64) * 3 + 7


def _make_call(nq, k, top, shift, seed):
    """One search result [nq,k] with the per-query cases of CASES dealt round-robin (starting at `shift`) -> D, I, qids, the
    qrels / addition dictionaries (pids) and the planted first-hit rank of every query (0 = none) for the qrels alone."""
    rs = np.random.RandomState(seed)
    D = np.full((nq, k), -np.inf, np.float32)
    I = np.full((nq, k), -1, np.int64)
    qids = (np.arange(nq, dtype=np.int64) * 5 + 11)
    pos_qp, pos_add, first_gold, cases = {}, {}, np.zeros(nq, np.int64), []
    for q in range(nq):
        case = CASES[(q + shift) % len(CASES)]
        cases.append(case)
        v = min(5, k) if case == "five_valid" else k
        rows = rs.choice(NCORPUS, size=v + 80, replace=False)
        ids, spare = rows[:v], rows[v:]                                  # spare rows: in the corpus, not in this result
        sc = np.sort((rs.randn(v) * 3 + 70).astype(np.float32))[::-1]
        if case == "ties":
            sc = np.sort(np.round(sc / 4) * 4)[::-1].astype(np.float32)   # a handful of distinct values
        D[q, :v], I[q, :v] = sc, ids
        t = min(top, v)
        gold, add = [], []
        if case == "rank0":
            gold = [ids[0]]
        elif case == "last":
            gold = [ids[t - 1]]
        elif case == "beyond_top":
            gold = [ids[rs.randint(top, v)]] if v > top else [spare[0]]
        elif case == "never":
            gold = [spare[0]]
        elif case == "seventy":                                           # more positives than a wavefront has lanes
            hit = sorted({0, t // 2, t - 1} | ({v - 1} if v > top else set()))
            gold = [ids[hit[-1]]] + list(spare[:30])
            add = list(spare[30:70 - len(hit)]) + [ids[h] for h in hit] + [gold[3]]      # (one repeats a qrels positive)
        elif case == "all_positive":
            gold, add = list(ids[:t:2]), list(ids[1:t:2])
        elif case == "five_valid":
            gold = [ids[min(2, v - 1)]]
        elif case == "ties":
            gold = [ids[t // 2]]
        elif case == "rank11":
            gold = [ids[min(10, v - 1)]]
        elif case == "rank51":
            gold = [ids[min(50, v - 1)]]
        if gold:
            pos_qp[int(qids[q])] = [int(p) for p in _pid(gold)]
            where = [int(np.flatnonzero(ids == g)[0]) for g in gold if g in ids]
            first_gold[q] = 1 + min(where) if where else 0
        if add:
            pos_add[int(qids[q])] = [int(p) for p in _pid(add)]
    return D, I, qids, pos_qp, pos_add, first_gold, cases


def _text_path(tmp_path, D, I, qids, pos_qp, pos_add, top):
    """write_to_file on the dictionaries get_question_topk builds, then the train side's parse -> per query (pos pairs, neg pairs)."""
    from simxns_amd.co_training.co_training_generate import write_to_file
    from simxns_amd.utils.MARCO_until_new import parse_pairs, read_sharded_tsv
    passage_ids = _pid(np.arange(NCORPUS))
    cand = {int(q): [int(passage_ids[j]) for j in I[r] if j >= 0] for r, q in enumerate(qids)}
    scores = {int(q): [float(s) for s, j in zip(D[r], I[r]) if j >= 0] for r, q in enumerate(qids)}
    path = write_to_file(cand, scores, [[int(q), "query %d" % q] for q in qids], pos_qp, pos_add, "train", str(tmp_path), 0)
    data = read_sharded_tsv(path)
    assert [int(s.query_id) for s in data] == [int(q) for q in qids]
    parsed = [(parse_pairs(s.pos_id) if s.pos_id else [], parse_pairs(s.neg_id) if s.neg_id else []) for s in data]
    return cand, parsed


@pytest.mark.parametrize("k,top", SHAPES)
@pytest.mark.parametrize("nq", [1, 37, 300])
def test_mine_negatives_equals_the_text_path(dev, tmp_path, nq, k, top):
    from simxns_amd import ops
    from simxns_amd.co_training.co_training_generate import compute_metrics
    from simxns_amd.mined_pool import metrics_from_first_hit, positives_csr
    assert min(top, k) == min(200, k)                                     # write_to_file cuts at 200: the shapes agree with it
    shift = SHAPES.index((k, top)) * 2 + (0 if nq > 1 else 1)
    D, I, qids, pos_qp, pos_add, first_gold, cases = _make_call(nq, k, top, shift, seed=nq * 7919 + k)
    passage_ids = _pid(np.arange(NCORPUS))
    cand, parsed = _text_path(tmp_path, D, I, qids, pos_qp, pos_add, top)
    ptr, rows = positives_csr(qids, pos_qp, pos_add, passage_ids)
    t = lambda a: torch.from_numpy(a).to(dev)
    out = {k_: v.cpu().numpy() for k_, v in ops.mine_negatives(t(D), t(I), t(ptr), t(rows), top=top).items()}
    assert out["neg_rows"].shape == out["neg_scores"].shape == (nq, top) and out["neg_rows"].dtype == np.int32
    want_rows = np.zeros((nq, top), np.int64)
    want_sc = np.full((nq, top), np.inf, np.float64)
    want_cnt = np.zeros(nq, np.int32)
    pad = np.ones((nq, top), bool)
    want_pos_pid, want_pos_sc = [], []
    for q, (pos, neg) in enumerate(parsed):
        c = len(neg)
        want_cnt[q] = c
        if c:
            want_rows[q, top - c:] = [p for p, _ in neg]
            want_sc[q, top - c:] = [s for _, s in neg]
            pad[q, top - c:] = False
        want_pos_pid += [p for p, _ in pos]
        want_pos_sc += [s for _, s in pos]
    assert np.array_equal(out["neg_cnt"], want_cnt)
    assert np.array_equal(np.where(pad, 0, passage_ids[out["neg_rows"]]), want_rows) and (out["neg_rows"][pad] == 0).all()
    assert np.array_equal(out["neg_scores"].astype(np.float64), want_sc)                    # the widening the pool loader does
    assert np.array_equal(out["neg_scores"].view(np.uint32), want_sc.astype(np.float32).view(np.uint32))
    assert [int(p) for p in passage_ids[rows]] == want_pos_pid                              # CSR order == the positive column's
    assert np.array_equal(out["pos_scores"].view(np.uint32), np.asarray(want_pos_sc, np.float64).astype(np.float32).view(np.uint32))
    # the cases did what they say
    for q, case in enumerate(cases):
        ps = out["pos_scores"][ptr[q]:ptr[q + 1]]
        if case in ("beyond_top", "never"):
            assert ps.tolist() == [0.0]
        if case == "all_positive":
            assert out["neg_cnt"][q] == 0 and (ps != 0).all()
        if case == "seventy":
            assert len(ps) >= 65 and 1 <= (ps != 0).sum() <= 3
        if case == "five_valid":
            assert out["neg_cnt"][q] == min(5, k) - 1
        if case == "none":
            assert len(ps) == 0 and out["neg_cnt"][q] == min(top, k) and out["first_hit"][q] == 0
    # first relevant rank against the qrels alone, over all k columns -> the metrics of compute_metrics
    gptr, grows = positives_csr(qids, pos_qp, {}, passage_ids)
    only = ops.mine_negatives(t(D), t(I), t(gptr), t(grows), top=top, want_negatives=False)
    assert set(only) == {"pos_scores", "first_hit"}
    fh = only["first_hit"].cpu().numpy()
    assert fh.dtype == np.int32 and np.array_equal(fh, first_gold)
    labelled = np.array([int(q) in pos_qp for q in qids])
    if labelled.any():
        assert metrics_from_first_hit(fh, labelled, len(pos_qp)) == compute_metrics(pos_qp, cand)
    else:
        with pytest.raises(IOError):
            metrics_from_first_hit(fh, labelled, len(pos_qp))
    if nq == 300 and k == 1000:                                           # the boundaries are really there
        got = {c: int(fh[cases.index(c)]) for c in ("rank11", "rank51", "beyond_top")}
        assert got["rank11"] == 11 and got["rank51"] == 51 and got["beyond_top"] > 200


def test_mine_negatives_bad_arguments_launch_nothing(dev):
    from simxns_amd import _lib as L
    from simxns_amd import ops
    lib = L.load()
    nq, k, top = 3, 8, 4
    D = torch.sort(torch.randn(nq, k, device=dev), descending=True).values
    I = torch.arange(nq * k, device=dev, dtype=torch.int64).view(nq, k)
    ptr = torch.tensor([0, 1, 1, 2], dtype=torch.int32, device=dev)
    pid = torch.tensor([2, 17], dtype=torch.int64, device=dev)
    SENT = 12345
    outs = dict(neg_rows=torch.full((nq, top), SENT, dtype=torch.int32, device=dev), neg_scores=torch.full((nq, top), float(SENT), device=dev),
                neg_cnt=torch.full((nq,), SENT, dtype=torch.int32, device=dev), pos_scores=torch.full((2,), float(SENT), device=dev),
                first_hit=torch.full((nq,), SENT, dtype=torch.int32, device=dev))

    def call(k_=k, top_=top, ids=I, **drop):
        o = {n: (None if n in drop else v) for n, v in outs.items()}
        rc = lib.simx_mine_negatives(L.stream_ptr(), nq, k_, top_, L.ptr(D), L.ptr(ids), L.ptr(ptr), L.ptr(pid), L.ptr(o["neg_rows"]),
                                     L.ptr(o["neg_scores"]), L.ptr(o["neg_cnt"]), L.ptr(o["pos_scores"]), L.ptr(o["first_hit"]))
        torch.cuda.synchronize()
        return rc

    def untouched():
        return all(bool((v == SENT).all()) for v in outs.values())

    BAD_SHAPE = -1
    assert call(k_=0) == BAD_SHAPE and untouched()
    assert call(k_=1025) == BAD_SHAPE and untouched()
    assert call(top_=0) == BAD_SHAPE and untouched()
    assert call(top_=1025) == BAD_SHAPE and untouched()
    assert call(neg_scores=1, neg_cnt=1) == BAD_SHAPE and untouched()     # only one of the three negative outputs
    assert call(neg_cnt=1) == BAD_SHAPE and untouched()
    big = I.clone()
    big[1, 3] = 2 ** 31
    assert call(ids=big) == BAD_SHAPE and untouched()
    assert "2^31" in lib.simx_last_error().decode()
    with pytest.raises(L.SimxError, match="2\\^31"):
        ops.mine_negatives(D, big, ptr, pid, top=top)
    with pytest.raises(ValueError):
        ops.mine_negatives(D, I, ptr[:-1], pid, top=top)
    # and the good call writes everything: 2^31 - 1 is a legal id, top > k is legal
    edge = I.clone()
    edge[0, 0] = 2 ** 31 - 1
    assert call(ids=edge) == 0 and not any(bool((v == SENT).any()) for v in outs.values())
    assert outs["neg_rows"][0].tolist() == [0, 2 ** 31 - 1, 1, 3] and outs["pos_scores"][0] == D[0, 2] and outs["first_hit"].tolist() == [3, 0, 2]
    wide = ops.mine_negatives(D, I, ptr, pid, top=k + 3)
    assert wide["neg_cnt"].tolist() == [k - 1, k, k - 1] and bool(torch.isinf(wide["neg_scores"][:, :3]).all())


# ---- end to end: generate job (both formats) -> the train job's dataset from either file -----------------------------------------------
def _write_corpus(root, n_pass=700, n_q=24):
    rs = np.random.RandomState(0)
    words = ["w%d" % i for i in range(300)]
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "para.txt"), "w") as f, open(os.path.join(root, "para.title.txt"), "w") as g:
        for pid in range(n_pass):
            f.write("%d\t%s\n" % (pid, " ".join(rs.choice(words, size=rs.randint(10, 60)))))
            g.write("%d\t%s\n" % (pid, " ".join(rs.choice(words, size=3))))
    with open(os.path.join(root, "train.query.txt"), "w") as f, open(os.path.join(root, "qrels.train.tsv"), "w") as g, \
            open(os.path.join(root, "qrels.train.addition.tsv"), "w") as h:
        for q in range(n_q):
            f.write("%d\t%s\n" % (q, " ".join("w%d" % w for w in rs.randint(0, 300, size=6))))
            gold = rs.randint(0, n_pass)
            g.write("%d 0 %d 1\n" % (q, gold))
            if q % 3 == 0:                                                # a second (and third) positive on some queries
                h.write("%d\t%d\n" % (q, (gold + 1 + rs.randint(0, n_pass - 1)) % n_pass))
            if q % 6 == 0:
                h.write("%d\t%d\n" % (q, (gold + 350) % n_pass))
            if q == 9:                                                    # repeats the qrels positive
                h.write("%d\t%d\n" % (q, gold))
    for name in ("student", "teacher"):
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        json.dump(dict(vocab_size=30522, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                       max_position_embeddings=192, type_vocab_size=2, layer_norm_eps=1e-12), open(os.path.join(d, "config.json"), "w"))


@pytest.fixture(scope="module")
def mined(dev, tmp_path_factory):
    """One generate run per format on the same model and corpus: `both` into gen/, `pool` into gen_pool/."""
    import types
    from simxns_amd.co_training import co_training_generate as Gn
    from simxns_amd.model.models import BiBertEncoder
    from simxns_amd.utils.MARCO_until_new import HashTokenizer
    base = tmp_path_factory.mktemp("mined")
    root = str(base / "data")
    _write_corpus(root)
    torch.manual_seed(3)
    args = types.SimpleNamespace(model_type=os.path.join(root, "student"), gradient_checkpointing=False, share_weight=False, fp16=True)
    model = BiBertEncoder(args).to(dev).eval()
    tok = HashTokenizer(model.question_model.config.vocab_size)
    gold = os.path.join(root, "qrels.train.tsv")
    pos, pos_add = Gn.load_pos_examples(gold, "train", root)
    assert len(pos_add) == 8 and pos_add[9][-1] == pos[9][0]
    runs = {}
    for fmt, name in (("both", "gen"), ("pool", "gen_pool")):
        out = str(base / name)
        os.makedirs(out)
        tools = Gn.RenewTools(os.path.join(root, "para.txt"), tok, out, os.path.join(root, "para.title.txt"), mined_format=fmt)
        index = tools.build_index(model, dev)
        result, path = tools.get_question_topk(model, dev, index, os.path.join(root, "train.query.txt"), gold, pos, pos_add, "train", 6)
        runs[fmt] = dict(out=out, tools=tools, result=result, path=path, pool=tools.pool_path)
    return dict(root=root, tok=tok, runs=runs, model=model)


def test_generate_job_formats(mined):
    from simxns_amd import mined_pool as MP
    from simxns_amd.co_training import co_training_generate as Gn
    both, pool = mined["runs"]["both"], mined["runs"]["pool"]
    assert both["path"] == os.path.join(both["out"], "train_ce_6.tsv") and both["pool"] == os.path.join(both["out"], "train_ce_6.pool.npz")
    assert pool["path"] == pool["pool"] == os.path.join(pool["out"], "train_ce_6.pool.npz")
    assert sorted(os.listdir(pool["out"])) == ["corpus_tok.json", "corpus_tok.r0of1.npy", "train_ce_6.pool.npz", "train_eval_result6.json"]
    # the metrics of the device path are those of compute_metrics on the host lists, to the last bit
    assert pool["result"] == both["result"] and pool["result"]["QueriesRanked"] == 24
    assert json.load(open(os.path.join(pool["out"], "train_eval_result6.json"))) == json.load(open(os.path.join(both["out"], "train_eval_result6.json")))
    a, b = MP.load_pool(both["pool"]), MP.load_pool(pool["pool"])
    assert a["meta"] == b["meta"] and a["meta"]["corpus_rows"] == 700 and a["meta"]["top"] == 200 and a["meta"]["corpus_slices"] == 1
    for k in MP.POOL_FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["pos_scores"] != 0).any() and (np.diff(a["pos_ptr"]) >= 2).sum() >= 8 and (a["neg_cnt"] >= 197).all()
    assert int(np.diff(a["pos_ptr"])[9]) == 2                             # qrels + one addition: the repeated positive adds no slot
    # the token table of the slice is reused by the next job on this --ann_dir
    again = Gn.RenewTools(os.path.join(mined["root"], "para.txt"), mined["tok"], pool["out"], os.path.join(mined["root"], "para.title.txt"),
                          mined_format="pool")
    assert isinstance(again.passage_table, np.memmap) and np.array_equal(again.passage_table, pool["tools"].passage_table)


@pytest.mark.parametrize("trainer_num", [1, 2])
def test_device_pool_from_the_pool_file_equals_the_text_path(dev, mined, trainer_num):
    from simxns_amd.utils.MARCO_until_new import Rocketqa_v2Dataset
    both, root, tok = mined["runs"]["both"], mined["root"], mined["tok"]
    for rank in range(trainer_num):
        kw = dict(num_hard_negatives=7, trainer_id=rank, trainer_num=trainer_num, corpus_path=root)
        text = Rocketqa_v2Dataset(both["path"], tok, **kw)
        binary = Rocketqa_v2Dataset(both["path"], tok, pool_path=both["pool"], **kw)
        assert len(text) == len(binary) == 24 // trainer_num
        P, B = text.build_device_pool(dev), binary.build_device_pool(dev)
        assert set(B) == {"q_tok", "p_tok", "cand_rows", "cand_scores", "pos_rows", "pos_scores", "pos_cnt", "device"}
        for k in ("q_tok", "cand_scores", "pos_scores", "pos_cnt"):      # the sampler sees the very table the text path gives it
            assert P[k].dtype == B[k].dtype and torch.equal(P[k], B[k]), k
        real = {"cand_rows": torch.isfinite(P["cand_scores"]),
                "pos_rows": torch.arange(P["pos_rows"].shape[1], device=dev)[None, :] < P["pos_cnt"][:, None]}
        for k in ("cand_rows", "pos_rows"):                               # row numbers differ, the tokens they name do not
            assert P[k].dtype == B[k].dtype and P[k].shape == B[k].shape and bool((B[k][~real[k]] == 0).all())
            assert torch.equal(P["p_tok"][P[k][real[k]].long()], B["p_tok"][B[k][real[k]].long()]), k
        assert P["p_tok"].shape == B["p_tok"].shape and P["p_tok"].dtype == B["p_tok"].dtype
        n = len(text)
        for indices in ([0, 3, 5, 9][:max(2, n // 3)], [n - 1, 1, n // 2, 7]):
            for step in (1, 2):
                x, y = text.device_batch(indices, seed=3, step=step), binary.device_batch(indices, seed=3, step=step)
                for part in ("student", "teacher"):
                    for u, w in zip(x[part], y[part]):
                        assert torch.equal(u, w) if torch.is_tensor(u) else u == w
                for name in x["lens"]:
                    assert torch.equal(x["lens"][name], y["lens"][name]), name
                assert torch.equal(x["picks"]["pos_choice"], y["picks"]["pos_choice"])


def test_pool_dataset_errors(dev, mined, tmp_path):
    from simxns_amd import mined_pool as MP
    from simxns_amd.utils.MARCO_until_new import HashTokenizer, Rocketqa_v2Dataset
    both, tok = mined["runs"]["both"], mined["tok"]
    with pytest.raises(ValueError, match="fewer than --number_neg 201"):
        Rocketqa_v2Dataset(both["path"], tok, num_hard_negatives=201, pool_path=both["pool"]).build_device_pool(dev)
    with pytest.raises(ValueError, match="mined with"):
        Rocketqa_v2Dataset(both["path"], HashTokenizer(1234), num_hard_negatives=7, pool_path=both["pool"]).build_device_pool(dev)
    a = MP.load_pool(both["pool"])
    lo, hi = a["pos_ptr"][4], a["pos_ptr"][5]                             # query 4 loses its positives
    ptr = a["pos_ptr"].copy()
    ptr[5:] -= hi - lo
    keep = np.r_[0:lo, hi:len(a["pos_rows"])]
    meta = {k: v for k, v in a["meta"].items() if k not in ("version", "top", "nq")}
    path = MP.save_pool(str(tmp_path / "train_ce_6.pool.npz"), a["qids"], a["q_tok"], a["neg_rows"], a["neg_scores"], a["neg_cnt"], ptr,
                        a["pos_rows"][keep], a["pos_scores"][keep], meta)
    with pytest.raises(ValueError, match="query 4 has no positive"):
        Rocketqa_v2Dataset(both["path"], tok, num_hard_negatives=7, pool_path=path).build_device_pool(dev)


def test_train_job_resumes_on_the_mined_pool(dev, mined, tmp_path):
    """The shell loop's second iteration with --mined_pool: after a first iteration on the text file, the train job at --global_step 4
    opens train_ce_4.pool.npz (--ann_dir holds no .tsv) and trains to the next boundary."""
    import shutil
    from simxns_amd.co_training import co_training_marco_train as T
    root, both = mined["root"], mined["runs"]["both"]
    out, ann = str(tmp_path / "ckpt"), str(tmp_path / "ann")
    os.makedirs(ann)
    shutil.copy(both["pool"], os.path.join(ann, "train_ce_4.pool.npz"))
    for name in ("corpus_tok.json", "corpus_tok.r0of1.npy"):
        shutil.copy(os.path.join(both["out"], name), os.path.join(ann, name))
    train = ["--model_type", os.path.join(root, "student"), "--teacher_model_type", os.path.join(root, "teacher"), "--tokenizer_name", "hash",
             "--output_dir", out, "--passage_path", root, "--ann_dir", ann, "--max_steps", "8", "--fp16", "--per_gpu_train_batch_size", "4",
             "--number_neg", "7", "--learning_rate", "1e-3", "--teacher_learning_rate", "1e-4", "--log_dir", str(tmp_path / "tb"),
             "--origin_data_dir", both["path"], "--logging_steps", "2", "--save_steps", "1000", "--iteration_step", "4",
             "--iteration_reranker_step", "2", "--temperature_distill", "1", "--num_workers", "0", "--sampler", "gpu", "--mined_pool"]
    assert T.main(train + ["--global_step", "0"]) == 4                   # (step 0 reads --origin_data_dir, a text file, as ever)
    assert T.main(train + ["--global_step", "4"]) == 8 and os.path.exists(os.path.join(out, "checkpoint-8"))
