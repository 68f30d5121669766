"""float16 storage of the flat index (FlatIPIndex(storage="fp16"), faiss's useFloat16) without a GPU: the C ABI's
declarations, the constructor's argument checks, the no-CPU-path error and the --index_float16 flag of the three generate
jobs.  No kernel is launched here; the numerics are tests/test_retrieval_f16_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("simx_ip_scores_f16", "simx_flat_ip_search_f16")


# ------------------------------------------------------------------------------------------ data shared with the GPU tests
# (nq, nc, H, k, chunk) of the exact-integer searches
INT_SHAPES = [(1, 129, 8, 10, 64), (130, 1000, 768, 200, 4096), (33, 5000, 776, 1000, 65536), (7, 150, 64, 200, 64),
              (64, 20000, 768, 200, 4096)]


def int_emb(seed, n, H):
    """integers of [-3, 3] as float32: exact in binary16, and every partial sum of a score is an integer of magnitude at most
    9 H < 2^24, hence exact in float32 in ANY accumulation order"""
    return np.random.RandomState(seed).randint(-3, 4, size=(n, H)).astype(np.float32)


def f16_emb(seed, n, H):
    """randn rounded to binary16 (round to nearest even), entries below the smallest normal 2^-14 zeroed, as float32"""
    x = np.random.RandomState(seed).randn(n, H).astype(np.float32).astype(np.float16).astype(np.float32)
    x[np.abs(x) < 2.0 ** -14] = 0.0
    return x


@pytest.mark.parametrize("nq,nc,H,k,chunk", INT_SHAPES[:4])
def test_oracle_is_exact_on_integer_data(nq, nc, H, k, chunk):
    """what lets the GPU test compare bit for bit: on int_emb the float32 fmaf chain of oracle/topk_ref.c has no rounding"""
    from oracle import retrieval as orr
    q, c = int_emb(nc, nq, H), int_emb(nc + 1, nc, H)
    exact = q.astype(np.float64) @ c.astype(np.float64).T                  # integers below 2^53: exact
    assert np.abs(exact).max() < 2.0 ** 24
    assert (orr.scores(q, c).astype(np.float64) == exact).all()
    assert (q.astype(np.float16).astype(np.float32) == q).all() and (c.astype(np.float16).astype(np.float32) == c).all()


def test_header_declares_and_library_exports_the_f16_entry_points():
    from simxns_amd import _lib as L
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simx.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in include/simx.h"
        assert name in L.SIGNATURES, name + " has no signature in simxns_amd/_lib.py"
        assert hasattr(lib, name), name + " is not exported by the built library"
    # same argument lists as the float32 entry points they mirror
    assert L.SIGNATURES["simx_ip_scores_f16"] == L.SIGNATURES["simx_ip_scores"]
    assert L.SIGNATURES["simx_flat_ip_search_f16"] == L.SIGNATURES["simx_flat_ip_search"]


def test_constructor_storage_argument():
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="fp16")
    assert ix.ntotal == 0 and ix.storage == "fp16"
    assert FlatIPIndex(64).storage == "fp32"                   # the default is the float32 index
    assert FlatIPIndex(12).storage == "fp32"                   # ... which keeps its dim % 4 rule
    with pytest.raises(ValueError):
        FlatIPIndex(12, storage="fp16")                        # rows must be 16-byte aligned: dim % 8 == 0
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="int8")


def test_no_cpu_path_fp16():
    from simxns_amd import _lib as L
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="fp16")
    with pytest.raises(L.SimxError):
        ix.add(torch.zeros(4, 64))
    with pytest.raises(L.SimxError):
        ix.search(torch.zeros(2, 64), 3)


def _parsers():
    from simxns_amd.Doc_training import co_training_doc_generate as doc
    from simxns_amd.co_training import co_training_generate as pas
    from simxns_amd.wiki import co_training_wiki_generate as wiki
    need = ["--model_type", "m", "--output_dir", "o", "--passage_path", "p"]
    return [("co_training_generate", pas.get_arguments, need), ("wiki", wiki.get_arguments, need), ("Doc_training", doc.get_arguments, need)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_generate_jobs_accept_index_float16(which):
    name, get_arguments, need = _parsers()[which]
    assert get_arguments(list(need)).index_float16 is False, name + ": --index_float16 must default to off"
    assert get_arguments(list(need) + ["--index_float16"]).index_float16 is True, name


def test_renew_tools_take_index_float16():
    import inspect
    from simxns_amd.Doc_training.co_training_generate_new_train import RenewTools as Doc
    from simxns_amd.co_training.co_training_generate import RenewTools as Pas
    from simxns_amd.wiki.co_training_generate_new_train_wiki import RenewTools as Wiki
    for cls in (Pas, Wiki, Doc):
        p = inspect.signature(cls.__init__).parameters
        assert "index_float16" in p and p["index_float16"].default is False, cls.__module__


def test_launch_passes_the_flag_to_the_generate_job_only(capsys):
    from simxns_amd import launch
    launch.main(["NQ", "--dry-run", "--last-step", "0"])
    assert "index_float16" not in capsys.readouterr().out      # off by default, in the NQ / TQ recipes as well
    launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_float16"])
    train, generate = capsys.readouterr().out.strip().splitlines()
    assert "--index_float16" in generate.split() and "index_float16" not in train
