"""Dense 3D U-Net between the two halves of the hot path (wiring, not a hot-path kernel).

`AtlasBackbone3D` refines the mean feature volume of the dense unprojection into multi-scale features for the TSDF
head whose finest output (`scene_tsdf_004`) drives the ray marching.  It is stock dense convolution work -- torch
Conv3d / BatchNorm3d, i.e. MIOpen on ROCm -- provided so that the `ray_marching_*` configs build with their
`backbone_3d` entry.  Sub-module and parameter names are the reference's (checkpoint keys `backbone3d.layers_down.1.0
.weight`, `...layers_up_res.0.1.bn2.running_var`, `...proj.0.conv.weight`; reference backbone3d.py:127-201), the
code is written from the architecture description:

  encoder level 0: `layers_down[0]` residual blocks at full resolution; level i > 0: 3x3x3 stride-2 conv + norm +
  ReLU, then residual blocks.  decoder step i: trilinear x2, 1x1x1 conv to the skip's width, projected skip
  (`proj[i]`: 1x1x1 conv [optionally kept only where the input volume was observed] + norm + ReLU), mean of the two,
  residual blocks.  Returns the decoder features coarse-to-fine.

`impl="device"` (opt-in; the default "torch" is the code path above, untouched) runs every 3x3x3 convolution of an eval-mode,
no-grad forward through cnrma_amd.unet instead: an implicit GEMM in the project's f16x3 arithmetic with the folded BatchNorm, the
residual sum and the ReLU in its epilogue.  The 1x1x1 convolutions, the up-sampling and the skip arithmetic stay torch ops.  In
training mode, or while a gradient is being recorded, the torch path runs.  Same parameter names and state-dict keys.

`joints="device"` (opt-in, needs impl="device"; the default "torch" is the paragraph above, bit for bit) also runs every decoder joint
-- up-sampling, both 1x1x1 convolutions, the conditional skip, its BatchNorm and ReLU, and the mean -- as one fused pass of
cnrma_amd.unet.join in exact fp32, and takes the observed mask and the input's magnitude bound from one pass over the input.  Each
joint publishes its output's bound, so the device forward measures no magnitude after the input's.
"""
import torch
from torch import nn
from torch.nn import functional as F

from ..registry import BACKBONES

_NORMS = {"BN": nn.BatchNorm3d, "GN": lambda c: nn.GroupNorm(32, c), "nnSyncBN": nn.SyncBatchNorm}


def make_norm(kind, channels):
    """'BN' | 'GN' | 'nnSyncBN' | '' (none) | a callable channels -> module"""
    if callable(kind):
        return kind(channels)
    return _NORMS[kind](channels) if kind else None


def _conv(cin, cout, k, stride=1):
    return nn.Conv3d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False)


class BasicBlock3d(nn.Module):
    """conv3-norm-ReLU-conv3-norm + identity, ReLU (dropout slots kept for key compatibility; p = `drop`)"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, drop=0, norm="BN"):
        super().__init__()
        self.conv1, self.bn1, self.drop1 = _conv(inplanes, planes, 3, stride), make_norm(norm, planes), nn.Dropout(drop, True)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2, self.drop2 = _conv(planes, planes, 3), make_norm(norm, planes), nn.Dropout(drop, True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = self.relu(self.drop1(self.bn1(self.conv1(x))))
        y = self.drop2(self.bn2(self.conv2(y)))
        y += x if self.downsample is None else self.downsample(x)
        return self.relu(y)


class ConditionalProjection(nn.Module):
    """skip connection: ReLU(norm(where(mask, conv1(enc), dec))) when `condition`, else ReLU(norm(conv1(enc)))"""

    def __init__(self, n, norm="BN", condition=True):
        super().__init__()
        self.conv, self.norm, self.relu = _conv(n, n, 1), make_norm(norm, n), nn.ReLU(True)
        self.condition = condition

    def forward(self, enc, dec, mask):
        s = self.conv(enc)
        if self.condition:
            s = torch.where(mask, s, dec)
        return self.relu(self.norm(s))


@BACKBONES.register_module()
class AtlasBackbone3D(nn.Module):
    def __init__(self, channels=(32, 64, 128), layers_down=(1, 2, 3), layers_up=(3, 3, 3), drop=0,
                 zero_init_residual=True, cond_proj=True, norm="BN", impl="torch", joints="torch"):
        super().__init__()
        if impl not in ("torch", "device"):
            raise ValueError(f"AtlasBackbone3D: impl must be 'torch' or 'device', got {impl!r}")
        if joints not in ("torch", "device"):
            raise ValueError(f"AtlasBackbone3D: joints must be 'torch' or 'device', got {joints!r}")
        if joints == "device" and impl != "device":
            raise ValueError(f"AtlasBackbone3D: joints='device' needs impl='device', got impl={impl!r}")
        self.impl, self.joints = impl, joints
        self.__dict__["_device_plan"] = None                        # (tag, runners) of the device path; never part of the state
        self.cond_proj = cond_proj
        L = len(channels)

        def blocks(c, n):
            return [BasicBlock3d(c, c, drop=drop, norm=norm) for _ in range(n)]

        downs, projs = [], []
        for i, c in enumerate(channels):
            head = [] if i == 0 else [_conv(channels[i - 1], c, 3, 2), make_norm(norm, c), nn.Dropout(drop, True),
                                      nn.ReLU(inplace=True)]
            downs.append(nn.Sequential(*head, *blocks(c, layers_down[i])))
            if i < L - 1:
                projs.append(ConditionalProjection(c, norm, cond_proj))
        self.layers_down = nn.ModuleList(downs)
        self.proj = nn.ModuleList(projs[::-1])                      # decoder order: deepest skip first
        up = list(channels)[::-1]
        self.layers_up_conv = nn.ModuleList([_conv(up[j - 1], up[j], 1) for j in range(1, L)])
        self.layers_up_res = nn.ModuleList([nn.Sequential(*blocks(up[j], layers_up[j - 1])) for j in range(1, L)])
        if zero_init_residual:                                      # residual branches start as identities
            for m in self.modules():
                if isinstance(m, BasicBlock3d):
                    nn.init.constant_(m.bn2.weight, 0)
        if impl == "device":
            self._check_device(norm)
        if joints == "device":
            self._check_joints(norm)

    # ---- impl="device": every 3x3x3 convolution, with its eval-mode BatchNorm, the residual sum and the ReLU, runs through
    # cnrma_amd.unet; the 1x1x1 convolutions, the up-sampling and the skip arithmetic stay torch ops unless joints="device" ----
    def _conv3_layers(self):
        """(name, conv, norm) of every 3x3x3 convolution, in forward order"""
        for group, levels in (("layers_down", self.layers_down), ("layers_up_res", self.layers_up_res)):
            for i, level in enumerate(levels):
                mods = list(level)
                if mods and not isinstance(mods[0], BasicBlock3d):
                    yield f"{group}.{i}.0", mods[0], mods[1]
                for j, m in enumerate(mods):
                    if isinstance(m, BasicBlock3d):
                        yield f"{group}.{i}.{j}.conv1", m.conv1, m.bn1
                        yield f"{group}.{i}.{j}.conv2", m.conv2, m.bn2

    def _check_device(self, norm):
        from cnrma_amd import unet
        if norm != "BN":
            raise ValueError(f"AtlasBackbone3D: impl='device' folds eval-mode BatchNorm3d and needs norm='BN', got norm={norm!r}")
        for name, conv, _ in self._conv3_layers():
            if not unet.widths_supported(conv.in_channels, conv.out_channels):
                raise ValueError(f"AtlasBackbone3D: impl='device' has no kernel for {name} ({conv.in_channels} -> "
                                 f"{conv.out_channels} channels): widths must be multiples of 32 up to 256")

    def _check_joints(self, norm):
        from cnrma_amd import unet
        if norm != "BN":
            raise ValueError(f"AtlasBackbone3D: joints='device' folds eval-mode BatchNorm3d and needs norm='BN', got norm={norm!r}")
        for i, (up, proj) in enumerate(zip(self.layers_up_conv, self.proj)):
            for name, conv in ((f"layers_up_conv.{i}", up), (f"proj.{i}.conv", proj.conv)):
                if not unet.widths_supported(conv.in_channels, conv.out_channels):
                    raise ValueError(f"AtlasBackbone3D: joints='device' has no kernel for {name} ({conv.in_channels} -> "
                                     f"{conv.out_channels} channels): widths must be multiples of 32 up to 256")

    def train(self, mode=True):
        self.__dict__["_device_plan"] = None          # writes through param.data (EMA hooks) bump no version counter
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.__dict__["_device_plan"] = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _device_tag(self):
        tag = tuple((t.data_ptr(), t._version) for _, conv, bn in self._conv3_layers()
                    for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))
        if self.joints == "device":
            tag += tuple((t.data_ptr(), t._version) for up, proj in zip(self.layers_up_conv, self.proj)
                         for t in (up.weight, proj.conv.weight, proj.norm.weight, proj.norm.bias, proj.norm.running_mean,
                                   proj.norm.running_var))
        return tag

    def _device_runners(self):
        """weight images and folded BatchNorm constants of every level, made once per set of weights: dropped by train(),
        load_state_dict() and any in-place update of a parameter or running statistic (version counters)"""
        from cnrma_amd import unet
        tag = self._device_tag()
        plan = self.__dict__["_device_plan"]
        if plan is None or plan[0] != tag:
            def level(seq):
                mods = list(seq)
                stem = unet.StemRunner(mods[0].weight, mods[1]) if mods and not isinstance(mods[0], BasicBlock3d) else None
                return stem, [unet.BlockRunner(m.conv1.weight, m.bn1, m.conv2.weight, m.bn2) for m in mods
                              if isinstance(m, BasicBlock3d)]
            joints = None
            if self.joints == "device":
                joints = [unet.JointRunner(up.weight, proj.conv.weight, proj.norm) for up, proj in zip(self.layers_up_conv, self.proj)]
            plan = (tag, [level(s) for s in self.layers_down], [level(s) for s in self.layers_up_res], joints)
            self.__dict__["_device_plan"] = plan
        return plan[1], plan[2], plan[3]

    def _use_device(self, x):
        if self.impl != "device" or self.training:
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    @staticmethod
    def _run_level(level, x, bound):
        stem, blocks = level
        if stem is not None:
            x, bound = stem(x, bound)
        for block in blocks:
            x, bound = block(x, bound)
        return x, bound

    def forward(self, x):
        device = self._use_device(x)
        joints, bound = None, None                                  # bound: the magnitude bound the last device layer published
        if device:
            downs, ups, joints = self._device_runners()
            x = x.contiguous()
        if joints is None:
            observed = (x != 0).any(1, keepdim=True).float() if self.cond_proj else None
        else:                                                       # one pass over the input: the mask and the first layer's bound
            from cnrma_amd import unet
            observed, bound = unet.observed_mask(x, with_bound=True) if self.cond_proj else (None, None)
        skips = []
        for i, layer in enumerate(self.layers_down):
            x, bound = self._run_level(downs[i], x, bound) if device else (layer(x), None)
            skips.append(x)
        skips.reverse()
        steps = len(self.layers_up_conv)
        out = []
        for i in range(steps):
            if joints is not None:                                  # the whole joint in one fused pass; its bound feeds the level
                x, bound = joints[i](x, skips[i + 1], observed, 2 ** (steps - i - 1))
                x = self._run_level(ups[i], x, bound)[0]
                out.append(x)
                continue
            x = self.layers_up_conv[i](F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False))
            mask = None
            if self.cond_proj:
                mask = F.interpolate(observed, scale_factor=1 / 2 ** (steps - i - 1)) != 0
            x = (x + self.proj[i](skips[i + 1], x, mask)) / 2
            x = self._run_level(ups[i], x, None)[0] if device else self.layers_up_res[i](x)
            out.append(x)
        return out
