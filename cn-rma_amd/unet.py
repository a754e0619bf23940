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
captured.  Inference only: no autograd."""
import torch

from . import _lib
from ._lib import CnrmaError, call_unet, ptr, stream

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
