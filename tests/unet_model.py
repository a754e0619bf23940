"""A host model of the f16x3 arithmetic of csrc/unet.hip, as csrc/f16x3.h and the kernel's header state it -- not a copy of the
kernel: no tiles, no LDS image, no accumulation order.

  s = 2^(14 - e), max|a| < 2^e           the power-of-two scale of an operand, from its largest magnitude (f16_scale_for)
  h = fp16(a s), m = fp16(a s - h)       both round to nearest; a s and a s - h are exact in fp32
  y = (conv(wm, xh) + conv(wh, xm) + conv(wh, xh)) / sx / sw      every product and the sum in fp64: the ideal result

and three mutants, each the slip the arithmetic invites: "drop_hm" (wh * xm missing), "drop_mh" (wm * xh missing), "swap_planes"
(the h and the m plane of the weight image exchanged).  tests/test_unet_model_cpu.py shows that the ideal model passes every bar
of the device tests and that the mutants do not."""
import copy
import math

import torch
import torch.nn.functional as F

from unet_cases import epilogue

MUTANTS = ("drop_hm", "drop_mh", "swap_planes")


def scale_for(amax):
    """f16_scale_for: 1 for 0, inf and nan; else 2^(14 - e) with amax < 2^e, the exponent clamped to [-100, 100]"""
    amax = float(amax)
    if not (amax > 0.0) or not (amax < 3.0e38):
        return 1.0
    return 2.0 ** max(-100, min(100, 14 - math.frexp(amax)[1]))


def split(a, s):
    """fp32 a, power-of-two s -> (h, m) as fp64 tensors holding fp16 values"""
    t = a.float() * s
    h = t.half()
    m = (t - h.float()).half()
    return h.double(), m.double()


def conv3(x, w, stride=1, mutant=None, bound=None, **kw):
    """the model's y in fp64, the epilogue (unet_cases.epilogue) composed in fp64; bound: an upper bound of max|x| (default: max|x|)"""
    assert mutant is None or mutant in MUTANTS
    sx = scale_for(x.abs().max() if bound is None else bound) if x.numel() else 1.0
    sw = scale_for(w.abs().max())
    xh, xm = split(x, sx)
    wh, wm = split(w, sw)
    if mutant == "swap_planes":
        wh, wm = wm, wh
    conv = lambda a, b: F.conv3d(b, a, stride=stride, padding=1)
    y = conv(wh, xh)
    if mutant != "drop_mh":
        y = y + conv(wm, xh)
    if mutant != "drop_hm":
        y = y + conv(wh, xm)
    return epilogue(y / sx / sw, **kw)


class ModelConv3(torch.nn.Module):
    """a 3x3x3 Conv3d of an fp64 module, computed by the model: the activation is the fp32 tensor the device would hold, its bound
    is its max|.| (what `absmax` and every layer's published bound are)"""

    def __init__(self, conv):
        super().__init__()
        self.weight, self.stride = conv.weight.detach().float(), conv.stride[0]

    def forward(self, x):
        return conv3(x.float(), self.weight, stride=self.stride)


def model_network(net64):
    """a copy of an fp64 AtlasBackbone3D whose 3x3x3 convolutions are the model; everything else stays fp64 torch"""
    net = copy.deepcopy(net64)
    for parent in list(net.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, torch.nn.Conv3d) and child.kernel_size == (3, 3, 3):
                setattr(parent, name, ModelConv3(child))
    return net
