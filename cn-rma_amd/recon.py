"""The TSDF regression head on the device (csrc/recon.hip, include/cnrma_recon.h; reference:
projects/mvsdetection/models/atlas_head.py:34-86).

    tsdf, loss = tsdf_head_scale(x, w, prev, threshold, label_smoothing, target=None)      # one scale
    output, losses = tsdf_head(xs, weights, thresholds, label_smoothing, targets=None)     # the module's two dicts

One scale is one forward launch (1x1x1 convolution, tanh, the +-0.999 fill from the previous scale) and, with a target, two loss
launches; the loss and its voxel count stay on the device, nothing is read back and nothing synchronises, so the calls run on the
current stream and can be captured.  x may be fp32, fp16 or bf16 and is read in place; dx comes back in x's dtype.  Gradients are
those autograd gives for the torch module: to x and w, none to prev or the target."""
import torch

from . import _lib
from ._lib import CnrmaError, call_recon, ptr, stream

ELEM = {torch.float32: _lib.RECON_CONSTANTS["CNRMA_RECON_ELEM_F32"], torch.float16: _lib.RECON_CONSTANTS["CNRMA_RECON_ELEM_F16"],
        torch.bfloat16: _lib.RECON_CONSTANTS["CNRMA_RECON_ELEM_BF16"]}


def _refuse(what):
    raise CnrmaError(f"tsdf_head_scale: {what} (invalid argument, {_lib.RECON_CONSTANTS['CNRMA_RECON_EINVAL']}); nothing was launched")


def _workspace(x):
    B, C, X, Y, Z = x.shape
    nbytes = _lib.load_recon().cnrma_recon_head_workspace_bytes(B, C, X, Y, Z)
    if nbytes == 0:
        _refuse(f"a feature volume of shape {tuple(x.shape)} is not supported")
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device), nbytes


def _prev_args(prev):
    return (None, 0, 0, 0) if prev is None else (ptr(prev), *prev.shape[2:])


class _HeadScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, prev, threshold, label_smoothing, target):
        B, C, X, Y, Z = x.shape
        tsdf = torch.empty((B, 1, X, Y, Z), dtype=torch.float32, device=x.device)
        call_recon("cnrma_recon_head_forward", ptr(x), ELEM[x.dtype], ptr(w), *_prev_args(prev), threshold, label_smoothing,
                   B, C, X, Y, Z, ptr(tsdf), stream())
        loss = dloss = count = None
        if target is not None:
            need_grad = any(ctx.needs_input_grad[:2])
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            count = torch.empty((), dtype=torch.int64, device=x.device)
            dloss = torch.empty_like(tsdf) if need_grad else None
            ws, nbytes = _workspace(x)
            call_recon("cnrma_recon_head_loss_f32", ptr(tsdf), *_prev_args(prev), threshold, ptr(target), B, X, Y, Z, ptr(ws),
                       nbytes, ptr(dloss), ptr(loss), ptr(count), stream())
        ctx.save_for_backward(x, w, prev, tsdf, dloss, count)
        ctx.scalars = (threshold, label_smoothing)
        ctx.set_materialize_grads(False)
        if count is not None:
            ctx.mark_non_differentiable(count)
        return tsdf, loss, count

    @staticmethod
    def backward(ctx, g_tsdf, g_loss, _g_count):
        x, w, prev, tsdf, dloss, count = ctx.saved_tensors
        threshold, label_smoothing = ctx.scalars
        B, C, X, Y, Z = x.shape
        want_x, want_w = ctx.needs_input_grad[:2]
        if g_loss is None or dloss is None:
            dloss = g_loss = None
        else:
            g_loss = g_loss.to(torch.float32).contiguous()
        if g_tsdf is not None:
            g_tsdf = g_tsdf.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty_like(w) if want_w else None
        ws, nbytes = _workspace(x) if want_w else (None, 0)
        call_recon("cnrma_recon_head_backward", ptr(x), ELEM[x.dtype], ptr(w), *_prev_args(prev), threshold, label_smoothing,
                   ptr(tsdf), ptr(g_tsdf), ptr(dloss), ptr(g_loss), ptr(count) if dloss is not None else None, B, C, X, Y, Z,
                   ptr(ws), nbytes, ptr(dx), ptr(dw), stream())
        return dx, dw, None, None, None, None


def _check(x, w, prev, target):
    _lib.require_gpu()
    if x.dim() != 5:
        _refuse(f"x must be [B, C, X, Y, Z], got shape {tuple(x.shape)}")
    if x.dtype not in ELEM:
        _refuse(f"x of {x.dtype} is not supported (float32, float16 or bfloat16)")
    if not x.is_contiguous():
        _refuse(f"x must be contiguous (shape {tuple(x.shape)}, strides {x.stride()})")
    B, C, X, Y, Z = x.shape
    if w.dtype != torch.float32 or w.numel() != C:
        _refuse(f"w must hold {C} float32 values, got {tuple(w.shape)} of {w.dtype}")
    if prev is not None and (prev.dtype != torch.float32 or prev.dim() != 5 or tuple(prev.shape[:2]) != (B, 1)
                             or tuple(2 * n for n in prev.shape[2:]) != (X, Y, Z)):
        _refuse(f"prev must be float32 [{B}, 1, X/2, Y/2, Z/2] with exactly half of x's grid {(X, Y, Z)}, got "
                f"{tuple(prev.shape)} of {prev.dtype}")
    if target is not None and (target.dtype != torch.float32 or tuple(target.shape) != (B, 1, X, Y, Z)):
        _refuse(f"the target must be float32 {(B, 1, X, Y, Z)}, got {tuple(target.shape)} of {target.dtype}")


def tsdf_head_scale(x, w, prev, threshold, label_smoothing, target=None, return_count=False):
    """One scale.  x [B,C,X,Y,Z] contiguous (fp32 / fp16 / bf16), w the decoder's C weights (fp32, any shape), prev the previous
    scale's output [B,1,X/2,Y/2,Z/2] (fp32) or None at the first scale, threshold = sparse_threshold of the previous scale
    (ignored without prev).  -> (tsdf [B,1,X,Y,Z] fp32, loss): loss is a device scalar, None without a target; with no voxel to
    average over it is NaN at the first scale and exactly 0 at the others.  return_count: also the voxel count (device int64)."""
    _check(x, w, prev, target)
    w1 = w.reshape(-1)
    if not w1.is_contiguous():
        w1 = w1.contiguous()
    prev = None if prev is None else prev.detach().contiguous()
    target = None if target is None else target.detach().contiguous()
    tsdf, loss, count = _HeadScale.apply(x, w1, prev, float(threshold), float(label_smoothing), target)
    return (tsdf, loss, count) if return_count else (tsdf, loss)


def tsdf_head(xs, weights, thresholds, label_smoothing, targets=None, keys=None):
    """The whole head, coarsest scale first: xs and weights per scale, thresholds[i - 1] sparsifies scale i.  keys: the voxel
    sizes in the dicts' names (default: 4 cm doubling towards the coarse end, '016', '008', '004' for three scales).
    -> ({'scene_tsdf_<key>': tsdf}, {'tsdf_loss_<key>': loss}) as AtlasTSDFHead.forward returns them; targets: {'tsdf_gt_<key>'}."""
    if keys is None:
        keys = [str(4 * 2 ** i).zfill(3) for i in reversed(range(len(xs)))]
    output, losses, prev = {}, {}, None
    for i, (x, w, key) in enumerate(zip(xs, weights, keys)):
        target = None if targets is None else targets["tsdf_gt_" + key]
        prev, loss = tsdf_head_scale(x, w, prev, thresholds[i - 1] if i else 0.0, label_smoothing, target)
        output["scene_tsdf_" + key] = prev
        if loss is not None:
            losses["tsdf_loss_" + key] = loss
    return output, losses
