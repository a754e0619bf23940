"""Host-side tests of the 3D U-Net decoder joints: the C surface of libcnrma_unetjoin_hip.so (include/cnrma_unet_join.h), its argument
checks (answered before any launch, so without a device), the module's `joints` keyword and its choice of path, and the host model
of the contract: on the GPU tests' own tensors the model and a plain fp32 torch composition pass the bar of tests/unet_join_cases.py,
and every plausible wrong reading of the contract fails it."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import unet_fixture as UF
import unet_join_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
JOIN_TABLE = {
    "cnrma_unet_join_abi_version": (I, []),
    "cnrma_unet_join_supported": (I, [I, I, I, I, I, I]),
    "cnrma_unet_join_scratch_bytes": (Z, [I, I, I, I, I, I]),
    "cnrma_unet_join_observed": (I, [P, I, I, I, I, I, P, P, P]),
    "cnrma_unet_join_forward": (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, P, P]),
}


def join_lib():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.UNET_JOIN_LIB_PATH):                              # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.UNET_JOIN_LIB_PATH), "-j8", "libcnrma_unetjoin_hip.so"], check=True)
    return _lib.load_unet_join()


def build(cond=False, impl="device", **over):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_backbone
    return build_backbone(dict(type="AtlasBackbone3D", cond_proj=cond, impl=impl, **dict(UF.NET, **over)))


def test_header_is_read_without_experiments():
    from cnrma_amd import _lib
    with open(_lib.UNET_JOIN_HEADER_PATH) as f:
        table, exp, constants = _lib._read_header(f.read())
    assert exp == {} and table == JOIN_TABLE and list(table) == list(JOIN_TABLE)
    assert _lib.UNET_JOIN_SIGNATURES == JOIN_TABLE
    assert constants == {"CNRMA_UNET_JOIN_EINVAL": -22, "CNRMA_UNET_JOIN_ABI_VERSION": 1, "CNRMA_UNET_JOIN_BOUND_WORDS": 1024}
    assert constants["CNRMA_UNET_JOIN_BOUND_WORDS"] == _lib.UNET_CONSTANTS["CNRMA_UNET_BOUND_WORDS"]
    assert len(_lib.SIGNATURES) == 128 and len(_lib.UNET_SIGNATURES) == 6        # the other surfaces are as they were
    assert not any(name.startswith("cnrma_unet_join") for name in list(_lib.SIGNATURES) + list(_lib.UNET_SIGNATURES))


def test_library_exports_exactly_the_header():
    from cnrma_amd import _lib
    lib = join_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.UNET_JOIN_LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}
    assert names == set(JOIN_TABLE)
    assert lib.cnrma_unet_join_abi_version() == 1
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "--check unet_join.resources.txt unetjoin_" in makefile
    assert "libcnrma_unetjoin_hip.so" in makefile.split("\nall:")[1].split("\n")[0]
    assert "libcnrma_unetjoin_hip.so" in makefile.split("\nclean:")[1] and "unet_join.o" in makefile.split("\nclean:")[1]
    assert "unet_join.resources.txt" in open(os.path.join(ROOT, ".gitignore")).read().split("\n")


def test_supported_shapes_and_scratch_size():
    from cnrma_amd import unet
    lib = join_lib()
    sup, nbytes = lib.cnrma_unet_join_supported, lib.cnrma_unet_join_scratch_bytes
    for c in (0, 16, 31, 32, 48, 64, 96, 128, 224, 256, 288, 512):
        for d in (32, 48, 256, 320):
            ok = c % 32 == 0 and 32 <= c <= 256 and d % 32 == 0 and d <= 256
            assert sup(1, c, d, 2, 3, 4) == int(ok) == int(unet.widths_supported(c, d)) and sup(1, d, c, 2, 3, 4) == int(ok)
            assert nbytes(2, c, d, 2, 3, 4) == (2 * d * 24 * 4 if ok else 0)
    assert sup(1, 64, 32, 96, 96, 40) == 1 and sup(1, 64, 32, 128, 128, 48) == 1 and sup(1, 32, 32, 1, 1, 1) == 1
    assert sup(1, 256, 256, 128, 128, 64) == 0                                   # out would hold 2^31 elements
    assert sup(1, 256, 256, 128, 128, 63) == 1
    for bad in ((0, 64, 32, 2, 2, 2), (1, 64, 32, 0, 2, 2), (1, 64, 32, 2, -1, 2), (1, 64, 32, 2, 2, 0), (70000, 32, 32, 1, 1, 1),
                (1, 32, 32, 1024, 1024, 256)):
        assert sup(*bad) == 0 and nbytes(*bad) == 0


FWD_ARGS = dict(xc=64, e=64, w_up=64, w_proj=64, scale=64, shift=64, observed=64, step=2, B=1, Cc=64, Cf=32, Xc=2, Yc=3, Zc=4,
                scratch=64, out=64, bound_out=64, stream=None)
FWD_BAD = [dict(Cc=48), dict(Cc=0), dict(Cc=288), dict(Cf=16), dict(Cf=320), dict(B=0), dict(Xc=0), dict(Yc=-1), dict(Zc=0),
           dict(Cc=256, Cf=256, Xc=128, Yc=128, Zc=64), dict(xc=None), dict(e=None), dict(w_up=None), dict(w_proj=None),
           dict(scratch=None), dict(out=None), dict(scratch=72), dict(step=0), dict(step=-2), dict(shift=None), dict(scale=None)]


@pytest.mark.parametrize("bad", FWD_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_forward_refuses_bad_arguments_before_any_launch(bad):
    """every refusal is answered on the host: the pointers are not even device pointers, so a launch would be a fault"""
    assert join_lib().cnrma_unet_join_forward(*dict(FWD_ARGS, **bad).values()) == -22


OBS_ARGS = dict(x=64, B=1, C=32, X=2, Y=3, Z=4, observed=64, bound_x=None, stream=None)
OBS_BAD = [dict(x=None), dict(observed=None), dict(B=0), dict(C=0), dict(X=0), dict(Y=-3), dict(Z=0), dict(B=70000),
           dict(C=256, X=2048, Y=2048, Z=2)]


@pytest.mark.parametrize("bad", OBS_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_observed_refuses_bad_arguments_before_any_launch(bad):
    assert join_lib().cnrma_unet_join_observed(*dict(OBS_ARGS, **bad).values()) == -22


def test_wrapper_needs_a_gpu_for_cpu_tensors():
    from cnrma_amd import unet
    from cnrma_amd._lib import CnrmaError
    k = C.make_case(64, 32, (1, 1, 1))
    with pytest.raises(CnrmaError, match="GPU|HIP device"):
        unet.join(k["xc"], k["e"], k["w_up"], k["w_proj"], k["scale"], k["shift"])
    with pytest.raises(CnrmaError, match="GPU|HIP device"):
        unet.observed_mask(k["xc"])


def test_joints_keyword():
    assert build().joints == "torch" and build(impl="torch").joints == "torch" and build(joints="device").joints == "device"
    with pytest.raises(ValueError, match="joints must be 'torch' or 'device', got 'triton'"):
        build(joints="triton")
    with pytest.raises(ValueError, match="joints='device' needs impl='device', got impl='torch'"):
        build(impl="torch", joints="device")
    with pytest.raises(ValueError, match="needs norm='BN', got norm='GN'"):
        build(impl="device", joints="device", norm="GN")
    assert list(build(impl="torch").state_dict()) == list(build(joints="device").state_dict())
    assert list(build(cond=True, impl="torch").state_dict()) == list(build(cond=True, joints="device").state_dict())


def test_joints_keyword_names_an_unsupported_width(monkeypatch):
    """the 3x3x3 check passes first (a width it refuses is refused as before); the 1x1x1 widths are then checked by name, without
    the library"""
    from cnrma_amd import _lib, unet

    def no_library(*a, **k):
        raise AssertionError("the device library was reached for")
    monkeypatch.setattr(_lib, "load_unet_join", no_library)
    monkeypatch.setattr(_lib, "load_unet", no_library)
    with pytest.raises(ValueError, match=r"no kernel for layers_down\.1\.0 \(32 -> 48 channels\)"):
        build(joints="device", channels=[32, 48, 128])
    real = unet.widths_supported
    monkeypatch.setattr(unet, "widths_supported", lambda cin, cout: cin == cout or cin < cout)       # every 3x3x3 layer, no up conv
    with pytest.raises(ValueError, match=r"joints='device' has no kernel for layers_up_conv\.0 \(128 -> 64 channels\)"):
        build(joints="device")
    monkeypatch.setattr(unet, "widths_supported", real)
    build(joints="device")


def test_training_and_grad_calls_take_the_torch_path_without_the_library(monkeypatch):
    from cnrma_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the device library was reached for")
    monkeypatch.setattr(_lib, "load_unet", no_library)
    monkeypatch.setattr(_lib, "load_unet_join", no_library)                      # call_unet_join goes through it too
    x = UF.make_input()
    ref, dev = UF.fill(build(cond=True, impl="torch")), UF.fill(build(cond=True, joints="device"))
    torch.manual_seed(0)
    exp = ref.train()(x)
    got = dev.train()(x)                                                         # training mode
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    exp = ref.eval()(x)
    got = dev.eval()(x)                                                          # eval mode, parameters record a gradient
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    dev.requires_grad_(False)
    got = dev(x.clone().requires_grad_(True))                                    # eval mode, the input records a gradient
    assert all(torch.equal(a, b) for a, b in zip(got, exp)) and got[0].requires_grad
    with pytest.raises((AssertionError, _lib.CnrmaError), match="reached for|HIP device|must live on the GPU"):
        with torch.no_grad():
            dev(x)                                                               # eval + no grad IS the device path


@pytest.mark.parametrize("cc,cf,dims,step", C.MODEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_host_model_and_torch_pass_the_bar_and_every_mutant_fails(cc, cf, dims, step):
    k = C.make_case(cc, cf, dims, 1, step)
    ref, mag = C.oracle(**k, step=step), C.magnitude(**k, step=step)
    bar = C.bar(mag, ref)
    assert 0 < C.max_error(C.host_model(**k, step=step), ref) <= bar             # the contract in fp32, commuted order
    assert 0 < C.max_error(C.oracle(**k, step=step, dtype=torch.float32), ref) <= bar          # the reference's lines in fp32
    plain = dict(k, observed=None)
    assert C.max_error(C.host_model(**plain), C.oracle(**plain)) <= C.bar(C.magnitude(**plain), C.oracle(**plain))
    for mutant in C.MUTANTS:
        assert C.max_error(C.host_model(**k, step=step, mutant=mutant), ref) > bar, mutant


@pytest.mark.parametrize("case", C.EXACT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_exact_inputs_leave_fp32_nothing_to_round(case):
    k = C.exact_case(*case)
    ref = C.oracle(**k, step=case[3])
    assert torch.equal(C.host_model(**k, step=case[3]).double(), ref) and torch.equal(ref.float().double(), ref)
    assert torch.equal(C.oracle(**k, step=case[3], dtype=torch.float32).double(), ref)
    assert float(ref.abs().max()) > 100 and float((ref == 0).double().mean()) < 0.5


def test_index_formula_equals_interpolate_in_fp64():
    g = torch.Generator().manual_seed(11)
    for dims in [(1, 1, 1), (1, 3, 2), (2, 3, 5), (5, 4, 9), (3, 2, 17)]:
        v = torch.randint(-2 ** 20, 2 ** 20, (2, 3, *dims), generator=g).double()        # integers: no order of summation rounds
        assert torch.equal(C.upsample(v), F.interpolate(v, scale_factor=2, mode="trilinear", align_corners=False))
        r = torch.randn(2, 3, *dims, generator=g, dtype=torch.float64)
        exp = F.interpolate(r, scale_factor=2, mode="trilinear", align_corners=False)
        assert float((C.upsample(r) - exp).abs().max()) <= 4 * 2.0 ** -53 * float(r.abs().max())
    i0, i1, lam = C.axis_taps(4)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert lam.tolist() == [0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]


@pytest.mark.parametrize("step", C.STEPS)
def test_strided_mask_equals_nearest_interpolate(step):
    g = torch.Generator().manual_seed(step)
    observed = (torch.rand(2, 6 * step, 4 * step, 10 * step, generator=g) < 0.6).to(torch.uint8)
    exp = F.interpolate(observed.float()[:, None], scale_factor=1 / step) != 0
    assert tuple(exp.shape) == (2, 1, 6, 4, 10) and torch.equal(exp, C.sampled_mask(observed, step))
    assert torch.equal(exp[:, 0], observed[:, ::step, ::step, ::step] != 0)
