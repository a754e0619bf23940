"""Restatement of one scale of the TSDF head (projects/mvsdetection/models/atlas_head.py; reference atlas_head.py:34-86) in plain
torch, in the precision the caller names: float64 is the oracle the device kernels (csrc/recon.hip) are measured against, float32
is the torch module's own arithmetic, line for line (tests/test_recon_cpu.py pins that the float32 chain IS the module's output).
Differentiable in x and w, so autograd of it in float64 is the gradient oracle.

The near / far choice is made on `prev` as it is given (float32, the dtype the head hands from scale to scale) in either precision,
so two implementations that get the same prev decide the same voxels."""
import torch
from torch.nn import functional as F

FILL = 0.999


def log_transform(x):
    return x.sign() * (1 + x.abs()).log()


def upsample(prev):
    """nearest x2: out[b, 0, x, y, z] = prev[b, 0, x >> 1, y >> 1, z >> 1]"""
    return prev.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)


def near_mask(prev, threshold):
    return upsample(prev.float()).abs() < threshold


def scale(x, w, prev, threshold, label_smoothing, target=None, dtype=torch.float64):
    """-> dict(tsdf, near, use, count, loss): tsdf [B,1,X,Y,Z] in `dtype`, near / use bool (near all true and use None without
    prev / target), count a Python int, loss a 0-d tensor in `dtype` (NaN for an empty first scale, 0.0 for an empty later one)"""
    C = x.shape[1]
    if dtype == torch.float32:
        y = F.conv3d(x.float(), w.float().reshape(1, C, 1, 1, 1))
    else:
        y = (x.to(dtype) * w.to(dtype).reshape(1, C, 1, 1, 1)).sum(1, keepdim=True)
    tsdf = torch.tanh(y) * label_smoothing
    near = torch.ones_like(tsdf, dtype=torch.bool)
    if prev is not None:
        up = upsample(prev.detach().float())
        near = up.abs() < threshold
        tsdf = torch.where(near, tsdf, (up.sign() * FILL).to(dtype))
    res = dict(tsdf=tsdf, near=near, use=None, count=None, loss=None)
    if target is not None:
        trgt = target.to(dtype)
        use = ((target < 1) | (target == 1).all(-1, keepdim=True)) & near
        err = (log_transform(tsdf) - log_transform(trgt)).abs()
        count = int(use.sum())
        loss = err[use].mean() if (prev is None or count) else 0 * err.sum()      # the mean of nothing is NaN
        res.update(use=use, count=count, loss=loss)
    return res


def chain(xs, ws, thresholds, label_smoothing, targets=None, dtype=torch.float64):
    """every scale, coarsest first; the output handed on is rounded to float32 as the head's is -> list of scale() dicts"""
    out, prev = [], None
    for i, (x, w) in enumerate(zip(xs, ws)):
        r = scale(x, w, prev, thresholds[i - 1] if i else 0.0, label_smoothing, None if targets is None else targets[i], dtype)
        out.append(r)
        prev = r["tsdf"].detach().float()
    return out
