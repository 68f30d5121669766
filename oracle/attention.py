"""float64 self-attention on the packed layout with the stateless dropout mask: the independent reference of the attention
kernels (simxns_amd/csrc/attention*.hip), forward and backward, with and without dropout on the probabilities.

TEST INFRASTRUCTURE (see oracle/__init__.py): imported only by tests/.

Per (sequence at packed offset t0 of n tokens, head h), with T the packed token count:
    mult = drop_multipliers(p, seed, stream, h*T + t0 + arange(n), arange(n))      (rows = head*T + query token, cols = key)
    P    = softmax(q k^T / sqrt(d))            lse = that of the UNDROPPED row
    ctx  = (P * mult) v
    dP   = (dO v^T) * mult                     dS = P * (dP - rowsum(dP * P)) / sqrt(d)
    dq   = dS k        dk = dS^T q             dv = (P * mult)^T dO
Without dropout every operation is the one of tests/test_kernels_gpu.py::_mha_ref in the same order: equal results.
"""
import math

import numpy as np

from . import bert as obert


def drop_mults(drop, T, h, t0, n):
    """-> (mf, mb) multipliers [n, n] of head h of the sequence at packed offset t0; drop = (p, seed, stream) or None.
    mf multiplies P (in ctx and in dv), mb multiplies dO v^T.  Here both are the one mask; tests that model a kernel fault pass
    mha_ref a `mults` of their own that returns two different ones."""
    if drop is None:
        return 1.0, 1.0
    p, seed, stream = drop
    m = obert.drop_multipliers(p, seed, stream, h * T + t0 + np.arange(n), np.arange(n))
    return m, m


def mha_ref(qkv, lens, heads, d, dctx=None, drop=None, mults=drop_mults):
    """qkv [T, 3*heads*d] float64 rows [q | k | v], lens the sequence lengths -> (ctx [T, H], lse [heads, T], dqkv [T, 3H] or None)."""
    T = qkv.shape[0]
    H = heads * d
    ctx = np.zeros((T, H))
    lse = np.zeros((heads, T))
    dqkv = np.zeros_like(qkv) if dctx is not None else None
    t0 = 0
    for n in lens:
        for h in range(heads):
            q = qkv[t0:t0 + n, h * d:(h + 1) * d]
            k = qkv[t0:t0 + n, H + h * d:H + (h + 1) * d]
            v = qkv[t0:t0 + n, 2 * H + h * d:2 * H + (h + 1) * d]
            mf, mb = mults(drop, T, h, t0, n)
            s = q @ k.T / math.sqrt(d)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            p = e / e.sum(1, keepdims=True)
            ctx[t0:t0 + n, h * d:(h + 1) * d] = (p * mf) @ v
            lse[h, t0:t0 + n] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
            if dctx is not None:
                do = dctx[t0:t0 + n, h * d:(h + 1) * d]
                dp = (do @ v.T) * mb
                ds = p * (dp - (dp * p).sum(1, keepdims=True)) / math.sqrt(d)
                dqkv[t0:t0 + n, h * d:(h + 1) * d] = ds @ k
                dqkv[t0:t0 + n, H + h * d:H + (h + 1) * d] = ds.T @ q
                dqkv[t0:t0 + n, 2 * H + h * d:2 * H + (h + 1) * d] = (p * mf).T @ do
        t0 += n
    return ctx, lse, dqkv
