"""One-pass float16 search of the flat index (FlatIPIndex(storage="fp16", fused=True)) without a GPU: the C ABI's declarations,
the workspace size, the constructor's argument checks, the no-CPU-path error and the --index_fused flag of the three generate
jobs and the launcher.  No kernel is launched here; the numerics are tests/test_retrieval_fused_gpu.py."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("simx_flat_ip_fused_workspace_bytes", "simx_ip_filter_f16", "simx_flat_ip_search_f16_fused")


def test_header_declares_and_library_exports_the_fused_entry_points():
    from simxns_amd import _lib as L
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simx.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS + ("simx_topk_fold_lists",):
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr), name + " is not declared in include/simx.h"
        assert name in L.SIGNATURES, name + " has no signature in simxns_amd/_lib.py"
        assert hasattr(lib, name), name + " is not exported by the built library"
    # the fused search = the unfused argument list + seed_rows, cand_cap after chunk and the overflow word at the end
    unfused = L.SIGNATURES["simx_flat_ip_search_f16"]
    res, args = L.SIGNATURES["simx_flat_ip_search_f16_fused"]
    assert res == unfused[0] and args[:9] == unfused[1][:9] and args[11:15] == unfused[1][9:] and len(args) == 16
    # every argument of the header's declaration has a ctypes type
    for name in NEW_SYMBOLS + ("simx_topk_fold_lists",):
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name


def test_workspace_grows_with_every_argument_and_holds_its_parts():
    from simxns_amd import _lib as L
    ws = L.load().simx_flat_ip_fused_workspace_bytes
    base = ws(128, 8192, 4096)
    assert ws(256, 8192, 4096) > base and ws(128, 16384, 4096) > base and ws(128, 8192, 8192) > base
    for nq, seed, cap in ((128, 8192, 4096), (1, 1, 1), (7, 130, 33), (8192, 8192, 4096)):
        # seed score block (f32) + candidate scores (f32) + candidate ids (int64) + counts (int32) + the overflow word
        parts = nq * seed * 4 + nq * cap * 4 + nq * cap * 8 + nq * 4 + 4
        assert ws(nq, seed, cap) >= parts, (nq, seed, cap)
        assert ws(nq, seed, cap) <= parts + nq * 12 + 128, "padding only: no hidden nq x chunk score block"


def test_constructor_fused_arguments():
    from simxns_amd.retrieval import FlatIPIndex
    assert inspect.signature(FlatIPIndex.__init__).parameters["fused"].default is False
    assert FlatIPIndex(64).fused is False and FlatIPIndex(64, storage="fp16").fused is False
    ix = FlatIPIndex(64, storage="fp16", fused=True)
    assert ix.fused is True and ix.cand_cap == 4096 and ix.seed_rows is None and ix.last_search_fallbacks == 0
    ix = FlatIPIndex(64, storage="fp16", fused=True, seed_rows=512, cand_cap=256)
    assert (ix.seed_rows, ix.cand_cap) == (512, 256)
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="fp32", fused=True)
    with pytest.raises(ValueError):
        FlatIPIndex(64, fused=True)                            # the default storage is float32
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="fp16", fused=True, cand_cap=0)
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="fp16", fused=True, seed_rows=0)


def test_no_cpu_path_fused():
    from simxns_amd import _lib as L
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="fp16", fused=True)
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
def test_generate_jobs_accept_index_fused(which, capsys):
    name, get_arguments, need = _parsers()[which]
    assert get_arguments(list(need)).index_fused is False, name + ": --index_fused must default to off"
    assert get_arguments(list(need) + ["--index_float16"]).index_fused is False, name
    args = get_arguments(list(need) + ["--index_float16", "--index_fused"])
    assert args.index_fused is True and args.index_float16 is True, name
    with pytest.raises(SystemExit) as e:                       # refused, with a message, without --index_float16
        get_arguments(list(need) + ["--index_fused"])
    assert e.value.code not in (0, None), name
    assert "index_float16" in (str(e.value.code) + capsys.readouterr().err), name + ": the refusal must say what is missing"


def test_renew_tools_take_index_fused():
    from simxns_amd.Doc_training.co_training_generate_new_train import RenewTools as Doc
    from simxns_amd.co_training.co_training_generate import RenewTools as Pas
    from simxns_amd.wiki.co_training_generate_new_train_wiki import RenewTools as Wiki
    for cls in (Pas, Wiki, Doc):
        p = inspect.signature(cls.__init__).parameters
        assert "index_fused" in p and p["index_fused"].default is False, cls.__module__
        with pytest.raises(ValueError):                        # checked before any file is read
            cls("/nonexistent", None, "/nonexistent", index_fused=True)


def test_launch_passes_the_flag_to_the_generate_job_only(capsys):
    from simxns_amd import launch
    launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_float16"])
    assert "index_fused" not in capsys.readouterr().out        # off by default
    launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_float16", "--index_fused"])
    train, generate = capsys.readouterr().out.strip().splitlines()
    assert "--index_fused" in generate.split() and "--index_float16" in generate.split() and "index_fused" not in train
    with pytest.raises(SystemExit) as e:
        launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_fused"])
    assert e.value.code not in (0, None) and "index_float16" in capsys.readouterr().err
