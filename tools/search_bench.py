"""Micro-benchmark of the generate job's search on one GPU (not part of bench.py's metric): inner-product scores + exact
top-k over a corpus shard resident in HBM, timed for BOTH index storages on the same corpus in one process -- float32 (one
fmaf chain per score, VALU) and float16 (binary16 rows, matrix cores) -- one JSON record each, then their ratio, then the kernels of one
default-size chunk (all queries x 65536 rows) timed apart by device events.
usage: python tools/search_bench.py [nq nc k] [--out FILE]"""
import json
import subprocess
import sys
import time

import torch

sys.path.insert(0, ".")
from simxns_amd import _lib as L                  # noqa: E402
from simxns_amd.retrieval import FlatIPIndex      # noqa: E402

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
nq, nc, k = (int(a) for a in argv[:3]) if len(argv) >= 3 else (2048, 1000000, 200)
H = 768
dev = torch.device("cuda:0")
torch.manual_seed(0)
parts = [torch.randn(min(250000, nc - lo), H, device=dev) for lo in range(0, nc, 250000)]
q = torch.randn(nq, H, device=dev)


def run(storage, repeats=3):
    index = FlatIPIndex(H, storage=storage)
    for p in parts:
        index.add(p)
    index.search(q[:64], k)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        index.search(q, k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = min(times)
    rate = 2.0 * nq * nc * H / dt
    return {"storage": storage, "nq": nq, "nc": nc, "k": k, "H": H, "seconds": round(dt, 4), "seconds_all": [round(t, 4) for t in times],
            "queries_per_s": round(nq / dt, 1), "tflops": round(rate / 1e12, 2),
            "score_bytes_per_s_tb": round(8.0 * nq * nc / dt / 1e12, 3),          # the score chunk is written, then read by the top-k
            "index_gb": round(nc * H * (2 if storage == "fp16" else 4) / 1e9, 3),
            "full_msmarco_train_job_s_per_gpu_of_8": round(502939 * 8841823 / 8 * H * 2 / rate, 1)}


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
    """the three kernels of one chunk pass, each alone: float16 scores, float32 scores, top-k update of a warm running set"""
    m = min(chunk, nc)
    c = parts[0][:m] if parts[0].shape[0] >= m else torch.cat(parts, 0)[:m]
    m = c.shape[0]
    q16, c16 = q.half(), c.half()
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
    ttk = ms(lambda: L.call("simx_topk_update", sp, nq, m, L.ptr(S), m, None, 0, 0, k, L.ptr(D), L.ptr(I)), 10)
    fl = 2.0 * nq * m * H
    return {"chunk": [nq, m, H], "ip_scores_f16_ms": round(t16, 3), "ip_scores_f16_tflops": round(fl / t16 / 1e9, 1),
            "ip_scores_f16_store_tb_s": round(nq * m * 4 / t16 / 1e9, 3), "ip_scores_f32_ms": round(t32, 3),
            "ip_scores_f32_tflops": round(fl / t32 / 1e9, 1), "topk_update_ms": round(ttk, 3), "topk_read_tb_s": round(nq * m * 4 / ttk / 1e9, 3)}


records = [run("fp32"), run("fp16")]
for r in records:
    print(json.dumps(r))
summary = {"fp32_seconds": records[0]["seconds"], "fp16_seconds": records[1]["seconds"],
           "fp16_speedup": round(records[0]["seconds"] / records[1]["seconds"], 2), "sclk": clock_mhz(),
           "device": torch.cuda.get_device_name(0)}
print(json.dumps(summary))
per_chunk = split()
print(json.dumps(per_chunk))
if out_path:
    with open(out_path, "w") as f:
        json.dump({"records": records, "summary": summary, "per_chunk": per_chunk}, f, indent=1)
        f.write("\n")
