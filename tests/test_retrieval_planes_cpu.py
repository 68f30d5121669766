"""Plane-pair storage of the flat index (FlatIPIndex(storage="planes")) without a GPU: the C ABI's declarations, the
constructor's argument checks, the no-CPU-path error, the --index_planes flag of the three generate jobs and the launcher, and
the premises of tests/test_retrieval_planes_gpu.py, checked here with NumPy.  No kernel is launched here.

Semantics (include/simx.h): a float32 value is held as hi = rnd16(x), lo = rnd16(x - hi) (binary16, nearest even) and a score is
the float32 accumulation of Qhi.Clo + Qlo.Chi + Qhi.Chi; lo.lo is dropped by definition."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import planes as oplanes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("simx_ip_scores_planes", "simx_ip_filter_planes", "simx_flat_ip_search_planes", "simx_flat_ip_search_planes_fused")
# each new entry point and the binary16 one whose argument list it takes, with (hi, lo) for each of the two 16-bit operands
NAMESAKES = {"simx_ip_scores_planes": "simx_ip_scores_f16", "simx_ip_filter_planes": "simx_ip_filter_f16",
             "simx_flat_ip_search_planes": "simx_flat_ip_search_f16", "simx_flat_ip_search_planes_fused": "simx_flat_ip_search_f16_fused"}


# ------------------------------------------------------------------------------------------ data shared with the GPU tests
# (nq, nc, H, k, chunk): ragged tiles in both directions, a K tail (776 = 12 x 64 + 8), several chunks, k > nc
SHAPES = [(1, 129, 8, 10, 64), (130, 1000, 768, 200, 4096), (33, 5000, 776, 1000, 65536), (7, 150, 64, 200, 64)]


def grid_emb(seed, n, H):
    """choice([-2, -1, 1, 2]) + randint(-1, 2) * 2^-12 as float32: hi is the integer, lo the multiple of 2^-12, and every
    partial sum of a three-term score is a multiple of 2^-12 below 2^12, hence exact in float32 in ANY accumulation order"""
    rs = np.random.RandomState(seed)
    return (rs.choice([-2.0, -1.0, 1.0, 2.0], size=(n, H)) + rs.randint(-1, 2, size=(n, H)) * 2.0 ** -12).astype(np.float32)


def split16(x):
    """the binary16 plane pair of a float32 array (oracle/planes.py), both planes as float32"""
    hi, lo = oplanes.split16(np.asarray(x), "f16")
    return hi.float().numpy(), lo.float().numpy()


def three_term(q, c):
    """Qhi.Clo + Qlo.Chi + Qhi.Chi in float64 (exact wherever the GPU tests compare bit for bit)"""
    qh, ql = (a.astype(np.float64) for a in split16(q))
    ch, cl = (a.astype(np.float64) for a in split16(c))
    return qh @ cl.T + ql @ ch.T + qh @ ch.T


def ranked(S, k, id_base=0):
    """(D, I) of the exact top-k of a score matrix: score descending, id ascending, padded with -inf / -1 beyond its columns"""
    nq, nc = S.shape
    D = np.full((nq, k), -np.inf, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for r in range(nq):
        order = np.lexsort((np.arange(nc), -S[r]))[:k]
        D[r, :len(order)] = S[r, order]
        I[r, :len(order)] = order + id_base
    return D, I


# ------------------------------------------------------------------------------------------ the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simx.h")).read(), flags=re.S)


def test_header_declares_the_planes_entry_points():
    hdr = _header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in include/simx.h"


def test_signatures_match_the_header_and_the_f16_namesakes():
    from simxns_amd import _lib as L
    hdr = _header()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name + " has no signature in simxns_amd/_lib.py"
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name
        res, args = L.SIGNATURES[name]
        fres, fargs = L.SIGNATURES[NAMESAKES[name]]
        # stream, three sizes, then (q, c) -> (q_hi, q_lo, c_hi, c_lo), then the namesake's remaining arguments unchanged
        assert res == fres and args[:4] == fargs[:4] and args[4:8] == [fargs[4]] * 2 + [fargs[5]] * 2 and args[8:] == fargs[6:], name


def test_library_exports_the_planes_entry_points():
    from simxns_amd import _lib as L
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported by the built library"


# ------------------------------------------------------------------------------------------ the constructor
def test_constructor_accepts_planes():
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="planes")
    assert ix.ntotal == 0 and ix.storage == "planes" and ix.fused is False
    assert inspect.signature(FlatIPIndex.__init__).parameters["storage"].default == "fp32"
    assert FlatIPIndex(64).storage == "fp32"                   # the default is still the float32 index
    with pytest.raises(ValueError):
        FlatIPIndex(12, storage="planes")                      # rows of a plane must be 16-byte aligned: dim % 8 == 0
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="int8")
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="plane")


def test_constructor_fused_with_planes():
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="planes", fused=True, seed_rows=512, cand_cap=256)
    assert ix.fused is True and (ix.seed_rows, ix.cand_cap) == (512, 256) and ix.last_search_fallbacks == 0
    assert FlatIPIndex(64, storage="fp16", fused=True).fused is True
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="fp32", fused=True)
    with pytest.raises(ValueError):
        FlatIPIndex(64, storage="planes", fused=True, cand_cap=0)


@pytest.mark.parametrize("fused", [False, True])
def test_no_cpu_path_planes(fused):
    from simxns_amd import _lib as L
    from simxns_amd.retrieval import FlatIPIndex
    ix = FlatIPIndex(64, storage="planes", fused=fused)
    with pytest.raises(L.SimxError):
        ix.add(torch.zeros(4, 64))
    with pytest.raises(L.SimxError):
        ix.search(torch.zeros(2, 64), 3)


# ------------------------------------------------------------------------------------------ the flags
def _parsers():
    from simxns_amd.Doc_training import co_training_doc_generate as doc
    from simxns_amd.co_training import co_training_generate as pas
    from simxns_amd.wiki import co_training_wiki_generate as wiki
    need = ["--model_type", "m", "--output_dir", "o", "--passage_path", "p"]
    return [("co_training_generate", pas.get_arguments, need), ("wiki", wiki.get_arguments, need), ("Doc_training", doc.get_arguments, need)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_generate_jobs_accept_index_planes(which, capsys):
    name, get_arguments, need = _parsers()[which]
    args = get_arguments(list(need))
    assert args.index_planes is False and args.index_float16 is False, name + ": --index_planes must default to off"
    assert get_arguments(list(need) + ["--index_float16"]).index_planes is False, name
    args = get_arguments(list(need) + ["--index_planes"])
    assert args.index_planes is True and args.index_float16 is False and args.index_fused is False, name
    args = get_arguments(list(need) + ["--index_planes", "--index_fused"])
    assert args.index_planes is True and args.index_fused is True and args.index_float16 is False, name
    with pytest.raises(SystemExit) as e:                       # one storage mode per index
        get_arguments(list(need) + ["--index_planes", "--index_float16"])
    assert e.value.code not in (0, None), name
    msg = str(e.value.code) + capsys.readouterr().err
    assert "index_planes" in msg and "index_float16" in msg, name + ": the refusal must name both flags"
    with pytest.raises(SystemExit) as e:                       # --index_fused alone is still refused, naming both modes
        get_arguments(list(need) + ["--index_fused"])
    msg = str(e.value.code) + capsys.readouterr().err
    assert e.value.code not in (0, None) and "index_float16" in msg and "index_planes" in msg, name


def test_renew_tools_take_index_planes():
    from simxns_amd.Doc_training.co_training_generate_new_train import RenewTools as Doc
    from simxns_amd.co_training.co_training_generate import RenewTools as Pas
    from simxns_amd.wiki.co_training_generate_new_train_wiki import RenewTools as Wiki
    for cls in (Pas, Wiki, Doc):
        p = inspect.signature(cls.__init__).parameters
        assert "index_planes" in p and p["index_planes"].default is False, cls.__module__
        with pytest.raises(ValueError):                        # both checked before any file is read
            cls("/nonexistent", None, "/nonexistent", index_planes=True, index_float16=True)
        with pytest.raises(ValueError):
            cls("/nonexistent", None, "/nonexistent", index_fused=True)
        with pytest.raises((OSError, IOError)):                # planes + fused passes the check and goes on to the files
            cls("/nonexistent", None, "/nonexistent", index_planes=True, index_fused=True)


def test_launch_passes_index_planes_to_the_generate_job_only(capsys):
    from simxns_amd import launch
    launch.main(["NQ", "--dry-run", "--last-step", "0"])
    assert "index_planes" not in capsys.readouterr().out       # off by default
    launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_planes"])
    train, generate = capsys.readouterr().out.strip().splitlines()
    assert "--index_planes" in generate.split() and "index_planes" not in train
    assert "index_float16" not in generate and "index_fused" not in generate
    launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_planes", "--index_fused"])
    train, generate = capsys.readouterr().out.strip().splitlines()
    assert "--index_planes" in generate.split() and "--index_fused" in generate.split() and "index_" not in train
    with pytest.raises(SystemExit) as e:
        launch.main(["NQ", "--dry-run", "--last-step", "0", "--index_planes", "--index_float16"])
    err = capsys.readouterr().err
    assert e.value.code not in (0, None) and "index_planes" in err and "index_float16" in err


# ------------------------------------------------------------------------------------------ premises of the GPU tests
def test_grid_data_splits_exactly_and_every_partial_sum_is_exact():
    nq, nc, H = SHAPES[1][:3]
    q, c = grid_emb(nc, nq, H), grid_emb(nc + 1, nc, H)
    for x in (q, c):
        hi, lo = split16(x)
        assert (hi == np.rint(x)).all() and np.isin(hi, [-2, -1, 1, 2]).all(), "hi is the integer part"
        assert (np.abs(lo) <= 2.0 ** -12).all() and (lo != 0).mean() > 0.6
        assert (hi.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all(), "hi + lo == x exactly"
        assert (hi * 4096 == np.rint(hi * 4096)).all() and (lo * 4096 == np.rint(lo * 4096)).all()      # products: multiples of 2^-12
    # |hi hi| <= 4, |hi lo| + |lo hi| <= 2^-10: the worst partial sum, in units of 2^-12, stays below 2^24 up to H = 776
    for H_ in (768, 776):
        assert H_ * (4 + 2.0 ** -10) * 2.0 ** 12 < 2.0 ** 24
    assert max(s[2] for s in SHAPES) <= 776
    S = three_term(q, c)
    assert (S * 4096 == np.rint(S * 4096)).all() and np.abs(S).max() * 4096 < 2.0 ** 24
    assert (S.astype(np.float32).astype(np.float64) == S).all(), "the expected scores are float32 numbers"


def test_grid_data_tells_the_three_terms_from_their_neighbours():
    """what the exact GPU comparison rejects: a kernel that scores hi.hi only, and one that also adds lo.lo (= the full product)"""
    nq, nc, H = SHAPES[1][:3]
    q, c = grid_emb(nc, nq, H), grid_emb(nc + 1, nc, H)
    S = three_term(q, c)
    hh = split16(q)[0].astype(np.float64) @ split16(c)[0].astype(np.float64).T
    full = q.astype(np.float64) @ c.astype(np.float64).T
    assert (S != hh).mean() > 0.90, "the corrections must show in most scores"
    assert (S != full).mean() > 0.75, "the dropped lo.lo term must show in most scores: the expected value is not q.c"


def test_split_error_model_on_random_data():
    rs = np.random.RandomState(3)
    for scale in (1.0, 0.05, 2.0 ** -13):
        x = (rs.randn(4096) * scale).astype(np.float32)
        hi, lo = split16(x)
        err = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
        assert (err <= np.maximum(2.0 ** -22 * np.abs(x.astype(np.float64)), 2.0 ** -25)).all()
