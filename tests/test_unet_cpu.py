"""Host-side tests of the device 3D U-Net convolutions: the C surface of libcnrma_unet_hip.so (include/cnrma_unet.h), its argument
checks (answered before any launch, so without a device), the module's `impl` keyword and its choice of path, the BatchNorm fold,
and the pin of tests/golden/atlas3d_wide.npz (made by tests/golden/make_golden_unet.py from the reference's AtlasBackbone3D) to
this repository's torch forward."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import unet_fixture as UF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
UNET_TABLE = {
    "cnrma_unet_abi_version": (I, []),
    "cnrma_unet_conv3_supported": (I, [I, I, I, I, I, I, I]),
    "cnrma_unet_conv3_weight_bytes": (Z, [I, I]),
    "cnrma_unet_conv3_prepare_weights": (I, [P, I, I, P, P]),
    "cnrma_unet_absmax_f32": (I, [P, L, P, P]),
    "cnrma_unet_conv3_forward": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P, P, P]),
}


def unet_lib():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.UNET_LIB_PATH):                                   # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.UNET_LIB_PATH), "-j8", "libcnrma_unet_hip.so"], check=True)
    return _lib.load_unet()


def build(cond=False, impl="torch", **over):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_backbone
    return build_backbone(dict(type="AtlasBackbone3D", cond_proj=cond, impl=impl, **dict(UF.NET, **over)))


def test_header_is_read_without_experiments():
    from cnrma_amd import _lib
    with open(_lib.UNET_HEADER_PATH) as f:
        table, exp, constants = _lib._read_header(f.read())
    assert exp == {} and table == UNET_TABLE and list(table) == list(UNET_TABLE)
    assert _lib.UNET_SIGNATURES == UNET_TABLE
    assert constants == {"CNRMA_UNET_EINVAL": -22, "CNRMA_UNET_ABI_VERSION": 1, "CNRMA_UNET_BOUND_WORDS": 1024}
    assert not any("debug" in name or "exp" in name for name in table)
    assert len(_lib.SIGNATURES) == 128                                           # the product surface is as it was
    assert not any(name.startswith("cnrma_unet_") for name in list(_lib.SIGNATURES) + list(_lib.EXPERIMENT_SIGNATURES))


def test_library_exports_exactly_the_header():
    from cnrma_amd import _lib
    lib = unet_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.UNET_LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}
    assert names == set(UNET_TABLE)
    for name in UNET_TABLE:
        assert getattr(lib, name) is not None
    assert lib.cnrma_unet_abi_version() == 1
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "--check unet.resources.txt unet_" in makefile and "libcnrma_unet_hip.so" in makefile.split("\nall:")[1].split("\n")[0]
    assert "unet.resources.txt" in open(os.path.join(ROOT, ".gitignore")).read()


def test_supported_shapes_and_image_size():
    from cnrma_amd import unet
    lib = unet_lib()
    for c in (0, 16, 31, 32, 48, 64, 96, 128, 224, 256, 288, 512):
        for d in (32, 48, 256, 320):
            ok = c % 32 == 0 and 32 <= c <= 256 and d % 32 == 0 and d <= 256
            assert (lib.cnrma_unet_conv3_weight_bytes(c, d) > 0) == ok == unet.widths_supported(c, d)
            assert lib.cnrma_unet_conv3_supported(1, c, d, 3, 3, 3, 1) == int(ok)
    assert lib.cnrma_unet_conv3_weight_bytes(32, 64) == 64 + 4 * 27 * 32 * 64     # the head + two fp16 halves per weight
    sup = lib.cnrma_unet_conv3_supported
    assert sup(1, 32, 32, 1, 1, 1, 1) == 1 and sup(1, 32, 32, 1, 1, 1, 2) == 1 and sup(2, 256, 256, 256, 256, 96, 1) == 0
    assert sup(1, 32, 32, 256, 256, 96, 1) == 1 and sup(1, 256, 256, 128, 128, 48, 1) == 1
    for bad in ((0, 32, 32, 4, 4, 4, 1), (1, 32, 32, 0, 4, 4, 1), (1, 32, 32, 4, -1, 4, 1), (1, 32, 32, 4, 4, 0, 2),
                (1, 32, 32, 4, 4, 4, 3), (1, 32, 32, 4, 4, 4, 0), (70000, 32, 32, 1, 1, 1, 1), (1, 32, 32, 2048, 2048, 512, 1)):
        assert sup(*bad) == 0


FWD_ARGS = dict(x=64, bound_x=64, image=64, scale=64, shift=64, residual=None, relu=1, stride=1, B=1, Cin=32, Cout=32, X=2, Y=3, Z=4,
                y=64, bound_y=64, stream=None)
FWD_BAD = [dict(Cin=48), dict(Cout=16), dict(Cout=288), dict(stride=3), dict(stride=0), dict(B=0), dict(X=0), dict(Z=-1), dict(x=None),
           dict(bound_x=None), dict(image=None), dict(y=None), dict(image=72), dict(shift=None), dict(X=2048, Y=2048, Z=512)]


@pytest.mark.parametrize("bad", FWD_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_forward_refuses_bad_arguments_before_any_launch(bad):
    """every refusal is answered on the host: the pointers are not even device pointers, so a launch would be a fault"""
    assert unet_lib().cnrma_unet_conv3_forward(*dict(FWD_ARGS, **bad).values()) == -22


def test_prepare_and_absmax_refuse_bad_arguments_before_any_launch():
    lib = unet_lib()
    for bad in ((None, 32, 32, 64, None), (64, 32, 32, None, None), (64, 48, 32, 64, None), (64, 32, 0, 64, None),
                (64, 32, 32, 68, None)):
        assert lib.cnrma_unet_conv3_prepare_weights(*bad) == -22
    for bad in ((None, 8, 64, None), (64, -1, 64, None), (64, 8, None, None)):
        assert lib.cnrma_unet_absmax_f32(*bad) == -22


def test_wrapper_needs_a_gpu_for_cpu_tensors():
    from cnrma_amd import unet
    from cnrma_amd._lib import CnrmaError
    with pytest.raises(CnrmaError, match="GPU|HIP device"):
        unet.prepare_conv3_weights(torch.zeros(32, 32, 3, 3, 3))


def test_impl_keyword():
    assert build().impl == "torch" and build(impl="device").impl == "device"
    with pytest.raises(ValueError, match="impl must be 'torch' or 'device', got 'triton'"):
        build(impl="triton")
    assert list(build().state_dict()) == list(build(impl="device").state_dict())
    with pytest.raises(ValueError, match="needs norm='BN', got norm='GN'"):
        build(impl="device", norm="GN")
    build(norm="GN")                                                             # the torch path takes any norm, as before
    with pytest.raises(ValueError, match=r"no kernel for layers_down\.1\.0 \(32 -> 48 channels\)"):
        build(impl="device", channels=[32, 48, 128])
    with pytest.raises(ValueError, match=r"no kernel for layers_down\.0\.0\.conv1 \(16 -> 16 channels\)"):
        build(impl="device", channels=[16, 32, 64])
    build(channels=[16, 32, 64])


def test_training_and_grad_calls_take_the_torch_path_without_the_library(monkeypatch):
    """the device path needs eval mode and no gradient being recorded; everything else is the torch forward, bit for bit, and never
    touches the library (this test has no device: reaching for it would raise)"""
    from cnrma_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the device library was reached for")
    monkeypatch.setattr(_lib, "load_unet", no_library)          # call_unet goes through it too
    x = UF.make_input()
    ref, dev = UF.fill(build(cond=True)), UF.fill(build(cond=True, impl="device"))
    torch.manual_seed(0)
    exp = ref.train()(x)
    ref_stats = {k: v.clone() for k, v in ref.state_dict().items()}
    got = dev.train()(x)                                                         # training mode
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    assert all(torch.equal(v, ref_stats[k]) for k, v in dev.state_dict().items())        # the running statistics moved alike
    exp = ref.eval()(x)
    got = dev.eval()(x)                                                          # eval mode, parameters record a gradient
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    dev.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    got = dev(xg)                                                                # eval mode, the input records a gradient
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    # eval + no grad IS the device path, and so is eval with nothing requiring a gradient: with CPU tensors it stops at the
    # missing device, or, where the machine has one, at the library this test took away
    with pytest.raises((AssertionError, _lib.CnrmaError), match="reached for|HIP device|must live on the GPU"):
        with torch.no_grad():
            dev(x)
    with pytest.raises((AssertionError, _lib.CnrmaError), match="reached for|HIP device|must live on the GPU"):
        dev(x)


@pytest.mark.parametrize("tag,cond", UF.CASES)
def test_torch_module_reproduces_the_fixture(tag, cond):
    """the fixture's outputs are the reference module's; this repository's forward, filled by the same keys, reproduces them"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "atlas3d_wide.npz"))
    x = UF.make_input()
    assert np.array_equal(x.numpy(), z["x"]) and tuple(x.shape) == UF.INPUT_SHAPE and not x[:, :, :3].any()
    net = UF.fill(build(cond=cond)).eval()
    with torch.no_grad():
        feats = net(x)
    assert len(feats) == 2
    for i, f in enumerate(feats):
        np.testing.assert_allclose(f.numpy(), z[f"{tag}_feat{i}"], rtol=1e-5, atol=1e-6)
        assert float(z[f"{tag}_fp32_error{i}"]) <= 1e-5                          # the reference's own fp32 error: 10x inside 1e-4
        assert 1.0 < float(np.abs(z[f"{tag}_feat{i}"]).max()) < 100.0            # O(1) activations


def test_fill_depends_on_the_key_and_the_salt_only():
    a, b, c = UF.fill(build()), UF.fill(build()), UF.fill(build(), salt="second")
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert not torch.equal(a.layers_down[0][0].conv1.weight, c.layers_down[0][0].conv1.weight)
    sd = a.state_dict()
    assert abs(float(sd["layers_down.0.0.bn1.weight"].mean()) - 1.0) < 0.1 and float(sd["layers_down.0.0.bn1.running_var"].min()) >= 0.5


def test_batchnorm_fold_equals_eval_batchnorm_in_fp64():
    from cnrma_amd import unet
    g = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm3d(64, eps=1e-3).double()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(64, generator=g)); bn.bias.copy_(torch.randn(64, generator=g))
        bn.running_mean.copy_(torch.randn(64, generator=g)); bn.running_var.copy_(0.1 + torch.rand(64, generator=g))
    x = torch.randn(2, 64, 3, 4, 5, generator=g, dtype=torch.float64)
    scale, shift = unet.fold_batchnorm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    assert scale.dtype == shift.dtype == torch.float32
    s64 = bn.weight / torch.sqrt(bn.running_var + bn.eps)                        # the fold as specified, in fp64 ...
    assert torch.equal(scale, s64.float()) and torch.equal(shift, (bn.bias - bn.running_mean * s64).float())
    with torch.no_grad():
        exp = bn.eval()(x)
    got = x * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    assert float((got - exp).abs().max()) <= 4 * 2.0 ** -24 * float(exp.abs().max())     # ... is eval BatchNorm up to the fp32 cast
    plain = torch.nn.BatchNorm3d(8, affine=False)
    plain.running_var.fill_(3.0); plain.running_mean.fill_(2.0)
    scale, shift = unet.fold_batchnorm(None, None, plain.running_mean, plain.running_var, plain.eps)
    assert torch.allclose(scale, torch.full((8,), (3.0 + 1e-5) ** -0.5)) and torch.allclose(shift, -2.0 * scale)
