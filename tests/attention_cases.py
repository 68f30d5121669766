"""What tests/test_attention_ref_cpu.py and tests/test_attention_edges_gpu.py share: the length lists, the inputs (plain and with
a key ramp), the dropout site, and the bounds -- as arrays of per-element limits, so that the CPU file can show on the float64
reference alone that these bounds see the faults the GPU file exists for.

None of the bounds is new.  Without dropout:
  "f32" / "bf16" / "f16"   test_mha_fwd_bwd's tol (ctx), lse bound and tolb (dqkv): |err| <= atol + rtol * |ref| per element;
  "pair"                   the plane-pair kernels (attention_x3.hip, and the planes form of the f32 unit it replaces, which writes
                           the same pair formats): test_mha_fwd_x3's 3e-6 * max(1, max|ctx|) and 2e-5 * max(1, max|lse|), and
                           test_mha_bwd_x3's 2e-5 * max(1, n / 256) * gmax per (sequence, head) block, gmax = the block's largest
                           |dq|, |dk| or |dv| of the reference.
With dropout every bound is multiplied by k = 256 / (256 - thr), the factor every kept probability carries
(test_mha_h16_dropout_rungs).  On ramped keys the dqkv bound of the first three is rtol * |ref| + atol * max(1, gmax / 3): 3 is
the block maximum of the unramped case (3.0 - 3.1), so the bound is the existing one scaled to the block, never tighter.
One bound is wider than its source: "planes" (the planes form of the f32 unit) is "pair" with 6e-6 instead of 3e-6 on ctx with
ramped keys, see limits().
"""
import numpy as np
import torch

from oracle import bert as obert
from oracle.attention import mha_ref

HEADS, D = 3, 64
SEED, STREAM = 0x9E3779B9, 19           # a seed with the high bit set; stream 19 is layer 1's attention site

LISTS = {
    "R2": [31, 9, 32, 1],                              # 2 tiles (h16, x3) / 1 tile (f32)
    "R8": [128, 1, 17, 33, 16, 100],                   # 8 / 4 tiles
    "R10": [160, 1, 129, 15, 45, 144],                 # 10 / 5 tiles (dense f32 form)
    "R16": [250, 1, 17, 5, 200, 33, 256, 161],         # 16 / 8 tiles with short sequences; chunked in x3
    "LONG": [300, 1, 33, 512, 129, 257, 128],          # chunked: ragged and exact chunks, one token past a chunk, a 1-token sequence
    "LONG2": [1030, 77],                               # 9 chunks
}

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}

TOL_CTX = {"f32": (2e-5, 2e-5), "bf16": (2e-2, 2e-2), "f16": (2.5e-3, 2.5e-3)}          # (rtol, atol)
TOL_LSE = {"f32": (1e-5, 2e-5), "bf16": (1e-5, 5e-3), "f16": (1e-5, 1e-3)}
TOL_DQKV = {"f32": (1e-4, 1e-4), "bf16": (3e-2, 6e-2), "f16": (4e-3, 8e-3)}


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32)


def rounded(a, fmt):
    """float32 array -> what a kernel of element format fmt sees, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH_DT[fmt]).to(torch.float64).numpy()


def inputs(lens, heads=HEADS, d=D, ramp=None, seeds=(1, 2)):
    """(qkv [T, 3H], dctx [T, H]) float32, drawn as in test_mha_fwd_bwd.  ramp "up" / "down": Q x 2 and the K row of in-sequence
    position j x (0.25 + 3.75 j / (n - 1)) (down: reversed; a 1-token sequence: 0.25) -- the row maximum sits in the last (first)
    chunk and the online softmax's running maximum rises (falls) chunk after chunk."""
    T, H = sum(lens), heads * d
    qkv, dctx = rnd((T, 3 * H), seeds[0]), rnd((T, H), seeds[1])
    if ramp is not None:
        qkv[:, :H] *= 2.0
        t0 = 0
        for n in lens:
            f = 0.25 + 3.75 * np.arange(n) / max(1, n - 1)
            if ramp == "down":
                f = f[::-1]
            qkv[t0:t0 + n, H:2 * H] *= f.astype(np.float32)[:, None]
            t0 += n
    return qkv, dctx


def drop_k(p):
    thr, _ = obert.drop_threshold(p)
    return 256.0 / (256.0 - thr)


def block_gmax(rdq, lens, heads, d):
    """[T, 3H] array: for every element the largest |dq|, |dk| or |dv| of the reference in its (sequence, head) block"""
    T, H = rdq.shape[0], heads * d
    a = np.abs(rdq).reshape(T, 3, heads, d)
    g = np.zeros((T, 1, heads, 1))
    t0 = 0
    for n in lens:
        g[t0:t0 + n] = a[t0:t0 + n].max(axis=(0, 1, 3), keepdims=True)
        t0 += n
    return np.broadcast_to(g, a.shape).reshape(T, 3 * H)


def limits(kind, ref, lens, heads, d, k=1.0, ramp=False):
    """per-element limits (ctx, lse, dqkv) of a kernel of kind "f32" / "bf16" / "f16" / "pair" / "planes" around the reference `ref` =
    (ctx, lse, dqkv); k = the dropout factor, ramp = the ramped-key form of the dqkv bound.  dqkv may be None."""
    rc, rl, rdq = ref
    if kind in ("pair", "planes"):
        # planes form on ramped keys: measured 1.047 x the 3e-6 bound (one element of 212544, LONG2 up; every other case <= 0.78),
        # round-off of f32 scores of magnitude 40 spread over all rows -- a plain float32 attention gives 0.67 - 1.10
        # (test_attention_ref_cpu.py).  Widened to 6e-6 (< 2 x 1.047 x 3e-6) for that unit and those inputs only.
        lc = np.full(rc.shape, (6e-6 if kind == "planes" and ramp else 3e-6) * max(1.0, np.abs(rc).max()))
        ll = np.full(rl.shape, 2e-5 * max(1.0, np.abs(rl).max()))
        lq = None
        if rdq is not None:
            nrow = np.repeat(np.asarray(lens, dtype=np.float64), lens)[:, None]
            lq = 2e-5 * np.maximum(1.0, nrow / 256.0) * block_gmax(rdq, lens, heads, d) + 1e-30
    else:
        (rt, at), (rtl, atl), (rtq, atq) = TOL_CTX[kind], TOL_LSE[kind], TOL_DQKV[kind]
        lc = at + rt * np.abs(rc)
        ll = atl + rtl * np.abs(rl)
        lq = None
        if rdq is not None:
            s = np.maximum(1.0, block_gmax(rdq, lens, heads, d) / 3.0) if ramp else 1.0
            lq = atq * s + rtq * np.abs(rdq)
    return lc * k, ll * k, None if lq is None else lq * k


def worst(got, ref, lim):
    """largest err / limit"""
    return float((np.abs(got - ref) / lim).max())


_REFS = {}


def reference(key, qkv, lens, heads, d, dctx, drop):
    """mha_ref on the values the kernel sees, computed once per key and left unchanged (the arrays are read-only); a hit must
    come with the same inputs."""
    hit = _REFS.get(key)
    if hit is None:
        out = mha_ref(qkv, lens, heads, d, dctx, drop)
        for a in out:
            a.setflags(write=False)
        hit = _REFS[key] = (qkv.copy(), dctx.copy(), out)
    assert np.array_equal(hit[0], qkv) and np.array_equal(hit[1], dctx), key
    return hit[2]
