"""What tests/golden/atlas3d_wide.npz is made of: the network, its input and a fill of its parameters that depends on their KEYS
only, so that tests/golden/make_golden_unet.py (the reference's module) and the tests (this repository's module) hold the same
weights without a weight fixture.

The fill keeps activations O(1) through the network -- every 1-D `*.weight` (the norm gains) is 1 + 0.1 r, which
helpers.fill_state_deterministic gives only to keys ending in `norm.weight`; with the convolution rule on `bn1.weight` the
activations reach 1e2 and the reference's own fp32 forward is 9e-5 from its fp64 forward, which leaves a 1e-4 criterion no room."""
import zlib

import torch

NET = dict(channels=[32, 64, 128], layers_down=[1, 1, 1], layers_up=[1, 1], zero_init_residual=False, norm="BN")
INPUT_SHAPE = (1, 32, 12, 20, 8)
CASES = (("plain", False), ("cond", True))


def fill(module, salt=""):
    """every floating tensor of the state dict <- a function of (salt + its key): crc32-seeded randn r; convolution weights
    r * sqrt(2 / fan_in); 1-D `*.weight` 1 + 0.1 r; `running_var` 0.5 + 0.5 |r|; every other 1-D tensor 0.1 r"""
    with torch.no_grad():
        for k, v in sorted(module.state_dict().items()):
            if not v.dtype.is_floating_point:
                continue
            g = torch.Generator().manual_seed(zlib.crc32((salt + k).encode()))
            r = torch.randn(v.shape, generator=g, dtype=torch.float32)
            if v.dim() > 1:
                r = r * (2.0 / max(1, v[0].numel())) ** 0.5
            elif k.endswith("running_var"):
                r = 0.5 + 0.5 * r.abs()
            elif k.endswith(".weight"):
                r = 1.0 + 0.1 * r
            else:
                r = 0.1 * r
            v.copy_(r)
    return module


def make_input():
    """O(1) values with an unobserved slab x[:, :, :3] = 0 (exercises the conditional projection and exact-zero halos)"""
    x = torch.randn(INPUT_SHAPE, generator=torch.Generator().manual_seed(20))
    x[:, :, :3] = 0
    return x
