"""The dense 3x3x3 convolutions of the Atlas 3D U-Net on the device (csrc/unet.hip, include/cnrma_unet.h; reference:
projects/mvsdetection/models/backbone3d.py:73-86).

    image = prepare_conv3_weights(weight)                                   # once per weight: fp16 fragment image + its scale
    y, bound_y = conv3(x, image, stride=1, scale=None, shift=None, residual=None, relu=False, bound=None)
    block = BlockRunner(conv1.weight, bn1, conv2.weight, bn2); y, bound_y = block(x, bound)         # a BasicBlock3d, eval mode
    stem = StemRunner(conv.weight, bn); y, bound_y = stem(x, bound)                                 # stride-2 conv + BN + ReLU

x and y are fp32 contiguous NCDHW; the arithmetic is the project's f16x3 (two fp16 planes per operand, three products, fp32
accumulation) with power-of-two scales from device-side magnitude bounds.  A bound is BOUND_WORDS fp32 words on the device (the
maximum of 64 slots); every convolution publishes its output's bound for the next layer, so a chain of layers needs one `absmax`
pass, over the network's input.  Nothing is read back and nothing synchronises: the calls run on the current stream and can be
captured.  Inference only: no autograd.

The decoder joints between the convolutions (csrc/unet_join.hip, include/cnrma_unet_join.h; reference backbone3d.py:188-196):

    observed = observed_mask(x)                                            # uint8 [B, X, Y, Z]: any over c of x != 0
    observed, bound_x = observed_mask(x, with_bound=True)                  # ... and x's magnitude bound from the same pass
    out, bound_out = join(xc, e, w_up, w_proj, scale, shift, observed=None, step=1)
    joint = JointRunner(up_conv.weight, proj.conv.weight, proj.norm); out, bound_out = joint(xc, e, observed, step)

out = (u + ReLU(scale * (observed ? p : u) + shift)) / 2 with u = w_up . trilinear_x2(xc) and p = w_proj . e, in exact fp32."""
import torch

from . import _lib
from ._lib import CnrmaError, call_unet, call_unet_join, ptr, stream

EINVAL = _lib.UNET_CONSTANTS["CNRMA_UNET_EINVAL"]
BOUND_WORDS = _lib.UNET_CONSTANTS["CNRMA_UNET_BOUND_WORDS"]


def _refuse(what):
    raise CnrmaError(f"conv3: {what} (invalid argument, {EINVAL}); nothing was launched")


def widths_supported(cin, cout):
    """whether a 3x3x3 convolution cin -> cout has a kernel: the header's rule (multiples of 32 in [32, 256]), restated so that a
    module can be checked at construction without loading the library; tests/test_unet_cpu.py holds it against
    cnrma_unet_conv3_weight_bytes"""
    return all(32 <= int(c) <= 256 and int(c) % 32 == 0 for c in (cin, cout))


class WeightImage:
    """a prepared 3x3x3 weight: `data` (device bytes: the scale and the fp16 fragments), cin, cout"""
    __slots__ = ("data", "cin", "cout")

    def __init__(self, data, cin, cout):
        self.data, self.cin, self.cout = data, cin, cout


def prepare_conv3_weights(weight):
    """weight [Cout, Cin, 3, 3, 3] fp32 on the device -> WeightImage.  max|w| is found on the device; two launches, no host read"""
    _lib.require_gpu()
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.dtype != torch.float32:
        _refuse(f"the weight must be float32 [Cout, Cin, 3, 3, 3], got {tuple(weight.shape)} of {weight.dtype}")
    cout, cin = weight.shape[:2]
    nbytes = _lib.load_unet().cnrma_unet_conv3_weight_bytes(cin, cout)
    if nbytes == 0:
        _refuse(f"widths {cin} -> {cout} are not supported (multiples of 32 up to 256)")
    w = weight.detach().contiguous()
    data = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call_unet("cnrma_unet_conv3_prepare_weights", ptr(w), cin, cout, ptr(data), stream())
    return WeightImage(data, cin, cout)


def absmax(x):
    """the magnitude bound of a contiguous fp32 device tensor: BOUND_WORDS words whose maximum is max|x| exactly"""
    _lib.require_gpu()
    if x.dtype != torch.float32 or not x.is_contiguous():
        _refuse(f"absmax needs a contiguous float32 tensor, got {tuple(x.shape)} of {x.dtype}, strides {x.stride()}")
    bound = torch.empty(BOUND_WORDS, dtype=torch.float32, device=x.device)
    call_unet("cnrma_unet_absmax_f32", ptr(x), x.numel(), ptr(bound), stream())
    return bound


def _vector(v, name, n, device):
    if v.dtype != torch.float32 or v.numel() != n or v.device != device:
        _refuse(f"{name} must hold {n} float32 values on {device}, got {tuple(v.shape)} of {v.dtype} on {v.device}")
    return v.detach().reshape(-1).contiguous()


def conv3(x, image, *, stride=1, scale=None, shift=None, residual=None, relu=False, bound=None, out=None):
    """y = conv3d(x, w, padding=1, stride=stride) in f16x3, then in fp32 and in this order: * scale[c] + shift[c], + residual, ReLU.
    x [B, Cin, X, Y, Z] fp32 contiguous; image = prepare_conv3_weights(w); bound: the magnitude bound of x (absmax(x), or the
    bound_y of the layer that wrote x; any upper bound of max|x| serves), computed here when None; out: a [B, Cout, X', Y', Z']
    fp32 contiguous tensor to write (allocated when None).  -> (y, bound_y), bound_y = max|y| in the same convention."""
    _lib.require_gpu()
    if not isinstance(image, WeightImage):
        _refuse("image must come from prepare_conv3_weights")
    if x.dim() != 5 or x.dtype != torch.float32:
        _refuse(f"x must be float32 [B, C, X, Y, Z], got {tuple(x.shape)} of {x.dtype}")
    if not x.is_contiguous():
        _refuse(f"x must be contiguous (shape {tuple(x.shape)}, strides {x.stride()})")
    B, C, X, Y, Z = x.shape
    if C != image.cin:
        _refuse(f"x has {C} channels, the weight image was prepared for {image.cin}")
    if stride not in (1, 2) or not _lib.load_unet().cnrma_unet_conv3_supported(B, C, image.cout, X, Y, Z, int(stride)):
        _refuse(f"a convolution {C} -> {image.cout} with stride {stride} over {tuple(x.shape)} is not supported")
    if (scale is None) != (shift is None):
        _refuse("scale and shift come together")
    shape = (B, image.cout, *((n - 1) // stride + 1 for n in (X, Y, Z)))
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device):
            _refuse(f"{name} must be contiguous float32 {shape} on {x.device}, got {tuple(t.shape)} of {t.dtype}, strides {t.stride()}")
    if bound is not None and (bound.dtype != torch.float32 or bound.numel() != BOUND_WORDS or bound.device != x.device):
        _refuse(f"bound must hold {BOUND_WORDS} float32 words on {x.device}")
    if scale is not None:
        scale, shift = _vector(scale, "scale", image.cout, x.device), _vector(shift, "shift", image.cout, x.device)
    x = x.detach()
    if bound is None:
        bound = absmax(x)
    y = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    bound_y = torch.empty(BOUND_WORDS, dtype=torch.float32, device=x.device)
    call_unet("cnrma_unet_conv3_forward", ptr(x), ptr(bound), ptr(image.data), ptr(scale), ptr(shift),
              None if residual is None else ptr(residual.detach()), int(bool(relu)), int(stride), B, C, image.cout, X, Y, Z, ptr(y),
              ptr(bound_y), stream())
    return y, bound_y


def fold_batchnorm(weight, bias, running_mean, running_var, eps):
    """eval-mode BatchNorm as a per-channel affine map: scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale,
    computed in fp64, returned in fp32.  weight / bias may be None (affine=False)"""
    var, mean = running_var.detach().double(), running_mean.detach().double()
    scale = torch.rsqrt(var + eps) if weight is None else weight.detach().double() / torch.sqrt(var + eps)
    shift = -mean * scale if bias is None else bias.detach().double() - mean * scale
    return scale.float().contiguous(), shift.float().contiguous()


class ConvBN:
    """one 3x3x3 convolution and the eval-mode BatchNorm behind it: the weight image and the folded (scale, shift), made once here"""

    def __init__(self, conv_weight, bn, stride=1):
        if bn.running_mean is None or bn.running_var is None:
            _refuse("the BatchNorm keeps no running statistics: there is no eval-mode map to fold")
        self.stride = stride
        self.image = prepare_conv3_weights(conv_weight)
        self.scale, self.shift = fold_batchnorm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)

    def __call__(self, x, bound=None, residual=None, relu=True):
        return conv3(x, self.image, stride=self.stride, scale=self.scale, shift=self.shift, residual=residual, relu=relu, bound=bound)


class BlockRunner:
    """BasicBlock3d in eval mode with an identity skip: ReLU(bn2(conv2(ReLU(bn1(conv1(x))))) + x), two launches"""

    def __init__(self, conv1_weight, bn1, conv2_weight, bn2):
        self.conv1, self.conv2 = ConvBN(conv1_weight, bn1), ConvBN(conv2_weight, bn2)

    def __call__(self, x, bound=None):
        y, b = self.conv1(x, bound)
        return self.conv2(y, b, residual=x)


class StemRunner(ConvBN):
    """the stride-2 stem of an encoder level: ReLU(bn(conv(x)))"""

    def __init__(self, conv_weight, bn):
        super().__init__(conv_weight, bn, stride=2)


# ---- the decoder joints: libcnrma_unetjoin_hip.so ----
def _refuse_join(what):
    raise CnrmaError(f"join: {what} (invalid argument, {_lib.UNET_JOIN_CONSTANTS['CNRMA_UNET_JOIN_EINVAL']}); nothing was launched")


def _volume(t, name):
    if t.dim() != 5 or t.dtype != torch.float32:
        _refuse_join(f"{name} must be float32 [B, C, X, Y, Z], got {tuple(t.shape)} of {t.dtype}")
    if not t.is_contiguous():
        _refuse_join(f"{name} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")


def observed_mask(x, with_bound=False):
    """x [B, C, X, Y, Z] fp32 contiguous -> observed uint8 [B, X, Y, Z] = (x != 0).any(1), read once; with_bound: -> (observed,
    bound_x), bound_x the magnitude bound of x (what absmax(x) gives) from the same pass"""
    _lib.require_gpu()
    _volume(x, "x")
    B, C, X, Y, Z = x.shape
    if min(B, C, X, Y, Z) < 1 or B > 65535 or x.numel() >= 2 ** 31:
        _refuse_join(f"a volume of shape {tuple(x.shape)} is not supported")
    x = x.detach()
    observed = torch.empty((B, X, Y, Z), dtype=torch.uint8, device=x.device)
    bound = torch.empty(BOUND_WORDS, dtype=torch.float32, device=x.device) if with_bound else None
    call_unet_join("cnrma_unet_join_observed", ptr(x), B, C, X, Y, Z, ptr(observed), ptr(bound), stream())
    return (observed, bound) if with_bound else observed


def join(xc, e, w_up, w_proj, scale, shift, observed=None, step=1, out=None, scratch=None):
    """one decoder joint.  xc [B, Cc, Xc, Yc, Zc], e [B, Cf, 2Xc, 2Yc, 2Zc], w_up [Cf, Cc] and w_proj [Cf, Cf] (any trailing 1s),
    scale / shift [Cf] (both None: no affine map), observed: None or uint8 [B, step 2Xc, step 2Yc, step 2Zc] (observed_mask of the
    network's input), everything fp32 contiguous on one device; out: a tensor like e to write (allocated when None); scratch: a
    uint8 buffer of cnrma_unet_join_scratch_bytes to reuse (allocated when None).  -> (out, bound_out), bound_out = max|out| in the
    convention conv3 takes as `bound`."""
    _lib.require_gpu()
    _volume(xc, "xc")
    _volume(e, "e")
    B, Cc, Xc, Yc, Zc = xc.shape
    Cf = e.shape[1]
    if e.shape[0] != B or tuple(e.shape[2:]) != (2 * Xc, 2 * Yc, 2 * Zc) or e.device != xc.device:
        _refuse_join(f"e must be [B, Cf, 2Xc, 2Yc, 2Zc] on {xc.device} for xc {tuple(xc.shape)}, got {tuple(e.shape)} on {e.device}")
    if not _lib.load_unet_join().cnrma_unet_join_supported(B, Cc, Cf, Xc, Yc, Zc):
        _refuse_join(f"a joint {Cc} -> {Cf} over {tuple(xc.shape)} is not supported")
    for name, w, cin in (("w_up", w_up, Cc), ("w_proj", w_proj, Cf)):
        if w.dtype != torch.float32 or w.dim() < 2 or tuple(w.shape[:2]) != (Cf, cin) or w.numel() != Cf * cin or w.device != xc.device:
            _refuse_join(f"{name} must be float32 [{Cf}, {cin}] on {xc.device}, got {tuple(w.shape)} of {w.dtype} on {w.device}")
        if not w.is_contiguous():
            _refuse_join(f"{name} must be contiguous (shape {tuple(w.shape)}, strides {w.stride()})")
    if (scale is None) != (shift is None):
        _refuse_join("scale and shift come together")
    if scale is not None:
        scale, shift = _vector(scale, "scale", Cf, xc.device), _vector(shift, "shift", Cf, xc.device)
    if observed is not None:
        if not isinstance(step, int) or step < 1:
            _refuse_join(f"step must be a positive integer, got {step!r}")
        want = (B, step * 2 * Xc, step * 2 * Yc, step * 2 * Zc)
        if observed.dtype != torch.uint8 or tuple(observed.shape) != want or not observed.is_contiguous() or observed.device != xc.device:
            _refuse_join(f"observed must be contiguous uint8 {want} on {xc.device}, got {tuple(observed.shape)} of {observed.dtype}, "
                         f"strides {observed.stride()}")
    if out is not None and (out.dtype != torch.float32 or out.shape != e.shape or not out.is_contiguous() or out.device != xc.device):
        _refuse_join(f"out must be contiguous float32 {tuple(e.shape)} on {xc.device}, got {tuple(out.shape)} of {out.dtype}, "
                     f"strides {out.stride()}")
    nbytes = _lib.load_unet_join().cnrma_unet_join_scratch_bytes(B, Cc, Cf, Xc, Yc, Zc)
    if scratch is None:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=xc.device)
    elif scratch.dtype != torch.uint8 or scratch.numel() < nbytes or not scratch.is_contiguous() or scratch.device != xc.device:
        _refuse_join(f"scratch must hold {nbytes} bytes (uint8) on {xc.device}")
    y = torch.empty_like(e) if out is None else out
    bound_out = torch.empty(BOUND_WORDS, dtype=torch.float32, device=xc.device)
    call_unet_join("cnrma_unet_join_forward", ptr(xc.detach()), ptr(e.detach()), ptr(w_up.detach()), ptr(w_proj.detach()), ptr(scale),
                   ptr(shift), ptr(observed), int(step), B, Cc, Cf, Xc, Yc, Zc, ptr(scratch), ptr(y), ptr(bound_out), stream())
    return y, bound_out


class JointRunner:
    """one decoder joint of the module in eval mode: layers_up_conv[i] (1x1x1), proj[i].conv (1x1x1) and proj[i].norm, folded once here.
    The weights are read as they lie (no prepared image); the scratch of the coarse product is kept between calls of one shape"""

    def __init__(self, up_weight, proj_weight, norm):
        if norm.running_mean is None or norm.running_var is None:
            _refuse_join("the BatchNorm keeps no running statistics: there is no eval-mode map to fold")
        self.w_up, self.w_proj = up_weight.detach().contiguous(), proj_weight.detach().contiguous()
        self.scale, self.shift = fold_batchnorm(norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)
        self.scratch = None

    def __call__(self, xc, e, observed=None, step=1):
        if xc.dim() == 5 and e.dim() == 5:
            nbytes = _lib.load_unet_join().cnrma_unet_join_scratch_bytes(xc.shape[0], xc.shape[1], e.shape[1], *xc.shape[2:])
            if self.scratch is None or self.scratch.numel() < nbytes or self.scratch.device != xc.device:
                self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=xc.device)
        return join(xc, e, self.w_up, self.w_proj, self.scale, self.shift, observed=observed, step=step, scratch=self.scratch)
