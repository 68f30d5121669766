"""Plane pairs ("operand planes", include/simx.h): the one CPU statement of the rule the device helpers of
simxns_amd/csrc/common.h (plane_split2 and friends) implement.

TEST INFRASTRUCTURE (see oracle/__init__.py): imported only by tests/, never by the product (the device path is
simxns_amd.retrieval.split_planes / simx_planes_from).

A float32 value x is held as two 16-bit values of one format,
    hi = rnd16(x),   lo = rnd16(x - hi)      (round to nearest even; the subtraction in float32)
and read back as hi + lo in float32.  A stored pair is NOT a fixed point of join-then-split: when x - hi rounds up to half an
ulp of hi, hi + lo is a tie and may round to the other neighbour.
"""
import numpy as np
import torch

FORMATS = {"f16": torch.float16, "bf16": torch.bfloat16, torch.float16: torch.float16, torch.bfloat16: torch.bfloat16}


def split16(x, fmt):
    """(hi, lo) of a float32 NumPy array or torch tensor, as CPU tensors of the 16-bit format.
    fmt: "f16" (binary16) / "bf16" (bfloat16), or the torch dtype."""
    t = FORMATS[fmt]
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32)) if isinstance(x, np.ndarray) else x.detach().cpu()
    assert x.dtype == torch.float32, x.dtype
    hi = x.to(t)
    lo = (x - hi.float()).to(t)
    return hi, lo


def join(hi, lo):
    """hi + lo in float32 (CPU tensor), what the device helpers plane_ld4 / plane_ld8 return"""
    return hi.detach().cpu().float() + lo.detach().cpu().float()
