"""Micro-benchmark of the generate job's search on one GPU (not part of bench.py's metric): inner-product scores + exact
top-k over a corpus shard resident in HBM, timed for the index storages on the same corpus in one process -- float32 (one
fmaf chain per score, VALU), planes and planes fused (binary16 plane pairs of the float32 rows, three MFMA terms; their searches
alternate with the float32 ones, which are their baseline), float16 (binary16 rows, matrix cores) and float16 fused (the one-pass
search; its searches alternate with the unfused float16 ones) -- one JSON record each, then their ratios, then the kernels of one
default-size chunk (all queries x 65536 rows) timed apart by device events: the unfused kernels, and the fused pairs at the warm
running set of a search's last chunk.
usage: python tools/search_bench.py [nq nc k] [--out FILE] [--planes-out FILE]"""
import json
import subprocess
import sys
import time

import torch

sys.path.insert(0, ".")
from simxns_amd import _lib as L                  # noqa: E402
from simxns_amd.retrieval import FlatIPIndex, split_planes      # noqa: E402

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
planes_out_path = None
if "--planes-out" in argv:
    i = argv.index("--planes-out")
    planes_out_path = argv[i + 1]
    del argv[i:i + 2]
nq, nc, k = (int(a) for a in argv[:3]) if len(argv) >= 3 else (2048, 1000000, 200)
H = 768
dev = torch.device("cuda:0")
torch.manual_seed(0)
parts = [torch.randn(min(250000, nc - lo), H, device=dev) for lo in range(0, nc, 250000)]
q = torch.randn(nq, H, device=dev)


def make_index(storage, fused=False):
    index = FlatIPIndex(H, storage=storage, fused=fused)
    for p in parts:
        index.add(p)
    return index


def run(indexes, repeats=3):
    """one record per index; the timed searches of several indexes alternate, so that they see the same clock and neighbours"""
    times, fallbacks = [[] for _ in indexes], [0] * len(indexes)
    for index in indexes:
        index.search(q[:64], k)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for i, index in enumerate(indexes):
            t0 = time.perf_counter()
            index.search(q, k)
            torch.cuda.synchronize()
            times[i].append(time.perf_counter() - t0)
            fallbacks[i] += index.last_search_fallbacks
    out = []
    for index, ts, fb in zip(indexes, times, fallbacks):
        dt = min(ts)
        rate = 2.0 * nq * nc * H / dt
        rec = {"storage": index.storage, "fused": index.fused, "nq": nq, "nc": nc, "k": k, "H": H, "seconds": round(dt, 4),
               "seconds_all": [round(t, 4) for t in ts], "queries_per_s": round(nq / dt, 1), "tflops": round(rate / 1e12, 2),
               "index_gb": round(nc * H * (2 if index.storage == "fp16" else 4) / 1e9, 3),      # planes: two binary16 planes
               "full_msmarco_train_job_s_per_gpu_of_8": round(502939 * 8841823 / 8 * H * 2 / rate, 1)}
        if index.fused:
            rec["last_search_fallbacks"] = fb                                   # summed over the timed searches
        else:
            rec["score_bytes_per_s_tb"] = round(8.0 * nq * nc / dt / 1e12, 3)   # the score chunk is written, then read by the top-k
        out.append(rec)
    return out


def clock_mhz():
    """current shader clock of GPU 0 as rocm-smi reports it (read only), or None"""
    try:
        txt = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        for key, val in json.loads(txt).get("card0", {}).items():
            if key.startswith("sclk clock speed"):
                return val
    except Exception:
        pass
    return None


def split(chunk=65536):
    """the kernels of one chunk pass, each alone: float16 scores, float32 scores, top-k update of a warm running set; then the
    fused pair on the LAST `chunk` rows of the corpus against the running set of all rows before them (the state a search is in
    there): the filter kernel, and the fold of the lists it wrote (the running set and the counts are restored before every fold;
    the restore is timed alone and subtracted)"""
    m = min(chunk, nc)
    c = parts[0][:m] if parts[0].shape[0] >= m else torch.cat(parts, 0)[:m]
    m = c.shape[0]
    q16, c16 = q.half(), c.half()
    qp, cp = split_planes(q), split_planes(c.contiguous())
    S = torch.empty(nq, m, device=dev)
    D = torch.full((nq, k), float("-inf"), device=dev)
    I = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    sp = L.stream_ptr()

    def ms(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    t32 = ms(lambda: L.call("simx_ip_scores", sp, nq, m, H, L.ptr(q), L.ptr(c), L.ptr(S), m), 3)
    t16 = ms(lambda: L.call("simx_ip_scores_f16", sp, nq, m, H, L.ptr(q16), L.ptr(c16), L.ptr(S), m), 10)
    tpl = ms(lambda: L.call("simx_ip_scores_planes", sp, nq, m, H, L.ptr(qp[0]), L.ptr(qp[1]), L.ptr(cp[0]), L.ptr(cp[1]), L.ptr(S), m), 10)
    ttk = ms(lambda: L.call("simx_topk_update", sp, nq, m, L.ptr(S), m, None, 0, 0, k, L.ptr(D), L.ptr(I)), 10)
    fl = 2.0 * nq * m * H
    fused = {}
    for storage in (("fp16", "planes") if nc > m else ()):
        head = FlatIPIndex(H, storage=storage)
        allrows = torch.cat(parts, 0)
        head.add(allrows[:nc - m])
        D0, I0 = head.search(q, k)
        tail = allrows[nc - m:].contiguous()
        qo, co = ((q16,), (tail.half(),)) if storage == "fp16" else (qp, split_planes(tail))
        operands = [L.ptr(t) for t in qo + co]
        name = "ip_filter_f16" if storage == "fp16" else "ip_filter_planes"
        del head, allrows, tail
        cap = 4096
        cs = torch.empty(nq, cap, device=dev)
        ci = torch.empty(nq, cap, dtype=torch.int64, device=dev)
        cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        D, I = D0.clone(), I0.clone()

        def filt():
            cnt.zero_()
            L.call("simx_" + name, sp, nq, m, H, *operands, nc - m, k, L.ptr(D0), L.ptr(I0), L.ptr(cs), L.ptr(ci), cap, L.ptr(cnt))

        def restore():
            D.copy_(D0); I.copy_(I0); cnt.copy_(cnt0)

        def fold():
            restore()
            L.call("simx_topk_fold_lists", sp, nq, L.ptr(cs), L.ptr(ci), cap, L.ptr(cnt), k, L.ptr(D), L.ptr(I), L.ptr(ovf))

        tfi = ms(filt, 10)
        cnt0 = cnt.clone()
        tz = ms(cnt.zero_, 10)
        tfo = ms(fold, 10)
        tre = ms(restore, 10)
        one = {"fused_chunk_rows_seen_before": nc - m, name + "_ms": round(tfi - tz, 3), name + "_tflops": round(fl / (tfi - tz) / 1e9, 1),
               "count_zero_ms_subtracted": round(tz, 4), "topk_fold_lists_ms": round(tfo - tre, 3), "restore_ms_subtracted": round(tre, 4),
               "survivors_per_query_mean": round(cnt0.float().mean().item(), 2), "survivors_per_query_max": int(cnt0.max().item()),
               "fold_overflows": int(ovf.item())}
        if storage == "fp16":
            fused.update(one)
        else:                                         # tflops of the planes kernels count 2 nq m H, the work of the product they stand for
            fused["planes"] = one
    return {"chunk": [nq, m, H], **fused, "ip_scores_f16_ms": round(t16, 3), "ip_scores_f16_tflops": round(fl / t16 / 1e9, 1),
            "ip_scores_f16_store_tb_s": round(nq * m * 4 / t16 / 1e9, 3), "ip_scores_f32_ms": round(t32, 3),
            "ip_scores_f32_tflops": round(fl / t32 / 1e9, 1), "ip_scores_planes_ms": round(tpl, 3),
            "ip_scores_planes_tflops": round(fl / tpl / 1e9, 1), "topk_update_ms": round(ttk, 3), "topk_read_tb_s": round(nq * m * 4 / ttk / 1e9, 3)}


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=30).stdout.strip() or None
    except Exception:
        return None


def same_result(a, b):
    """do two indexes return the same bits for the benchmark's queries?"""
    (Da, Ia), (Db, Ib) = a.search(q, k), b.search(q, k)
    return bool((Ia == Ib).all().item() and (Da.view(torch.int32) == Db.view(torch.int32)).all().item())


f16, fus = make_index("fp16"), make_index("fp16", fused=True)
same = same_result(f16, fus)
pl, plf = make_index("planes"), make_index("planes", fused=True)
same_planes = same_result(pl, plf)
r32 = run([make_index("fp32"), pl, plf])              # the float32 baseline of the planes rows is timed between them
del pl, plf
records = r32[:1] + run([f16, fus]) + r32[1:]
del f16, fus
for r in records:
    print(json.dumps(r))
summary = {"fp32_seconds": records[0]["seconds"], "fp16_seconds": records[1]["seconds"], "fp16_fused_seconds": records[2]["seconds"],
           "fp16_speedup": round(records[0]["seconds"] / records[1]["seconds"], 2),
           "fused_speedup_over_fp16": round(records[1]["seconds"] / records[2]["seconds"], 2),
           "fused_result_equals_fp16_bit_for_bit": same, "last_search_fallbacks": records[2]["last_search_fallbacks"],
           "planes_seconds": records[3]["seconds"], "planes_fused_seconds": records[4]["seconds"],
           "planes_speedup_over_fp32": round(records[0]["seconds"] / records[3]["seconds"], 2),
           "planes_fused_speedup_over_fp32": round(records[0]["seconds"] / records[4]["seconds"], 2),
           "planes_fused_result_equals_planes_bit_for_bit": same_planes, "planes_last_search_fallbacks": records[4]["last_search_fallbacks"],
           "sclk": clock_mhz(), "commit": commit(), "device": torch.cuda.get_device_name(0)}
print(json.dumps(summary))
per_chunk = split()
print(json.dumps(per_chunk))
for path, recs in ((out_path, records), (planes_out_path, [records[0], records[3], records[4]])):
    if path:
        with open(path, "w") as f:
            json.dump({"records": recs, "summary": summary, "per_chunk": per_chunk}, f, indent=1)
            f.write("\n")
