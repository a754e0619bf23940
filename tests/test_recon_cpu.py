"""Host-side tests of the device TSDF head: the C surface of libcnrma_recon_hip.so (include/cnrma_recon.h), its argument checks
(answered before any launch, so without a device), and the first pin of the head's fill branch and loss to the reference:
tests/golden/tsdf_head.npz (made by tests/golden/make_golden_tsdf_head.py from the reference's AtlasTSDFHead run WITH targets)
against the float64 oracle tests/recon_oracle.py and against the project's own torch module."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import recon_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
RECON_TABLE = {
    "cnrma_recon_abi_version": (I, []),
    "cnrma_recon_head_workspace_bytes": (Z, [I, I, I, I, I]),
    "cnrma_recon_head_forward": (I, [P, I, P, P, I, I, I, F, F, I, I, I, I, I, P, P]),
    "cnrma_recon_head_loss_f32": (I, [P, P, I, I, I, F, P, I, I, I, I, P, Z, P, P, P, P]),
    "cnrma_recon_head_backward": (I, [P, I, P, P, I, I, I, F, F, P, P, P, P, P, I, I, I, I, I, P, Z, P, P, P]),
}
CASES = ("mixed", "allfar", "allnear", "empty0")
KEYS = ("016", "008", "004")
TOL = 1e-4                      # the project's parity bound


def recon_lib():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.RECON_LIB_PATH):                                  # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.RECON_LIB_PATH), "-j8", "libcnrma_recon_hip.so"], check=True)
    return _lib.load_recon()


def load_case(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tsdf_head.npz"))
    pick = lambda what: [torch.from_numpy(z[f"{name}_{what}{i}"]) for i in range(3)]
    return dict(xs=pick("x"), ws=pick("w"), targets=pick("gt"), tsdfs=pick("tsdf"), losses=pick("loss"),
                label_smoothing=float(z["label_smoothing"]), thresholds=[float(t) for t in z["thresholds"]])


def same_loss(got, ref, tol=TOL):
    """NaN where the reference has NaN, the exact +0.0 where it has it, within tol elsewhere"""
    got, ref = float(got), float(ref)
    if np.isnan(ref):
        return np.isnan(got)
    if ref == 0.0:
        return got == 0.0 and not np.signbit(got)
    return abs(got - ref) <= tol


def test_header_is_read_without_experiments():
    from cnrma_amd import _lib
    with open(_lib.RECON_HEADER_PATH) as f:
        table, exp, constants = _lib._read_header(f.read())
    assert exp == {} and table == RECON_TABLE and list(table) == list(RECON_TABLE)
    assert _lib.RECON_SIGNATURES == RECON_TABLE
    assert constants == {"CNRMA_RECON_EINVAL": -22, "CNRMA_RECON_ABI_VERSION": 1, "CNRMA_RECON_ELEM_F32": 0,
                         "CNRMA_RECON_ELEM_F16": 1, "CNRMA_RECON_ELEM_BF16": 2} and _lib.RECON_ABI_VERSION == 1
    assert constants["CNRMA_RECON_ELEM_F16"] == _lib.CONSTANTS["CNRMA_ELEM_F16"]
    assert constants["CNRMA_RECON_ELEM_BF16"] == _lib.CONSTANTS["CNRMA_ELEM_BF16"]
    assert not any("debug" in name or "exp" in name for name in table)
    assert len(_lib.SIGNATURES) == 128                                           # the product surface is as it was
    assert not any(name.startswith("cnrma_recon_") for name in list(_lib.SIGNATURES) + list(_lib.EXPERIMENT_SIGNATURES))


def test_library_exports_exactly_the_header():
    from cnrma_amd import _lib
    lib = recon_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.RECON_LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}
    assert names == set(RECON_TABLE)
    for name in RECON_TABLE:
        assert getattr(lib, name) is not None
    assert lib.cnrma_recon_abi_version() == 1
    if os.path.exists(_lib.LIB_PATH):                                            # the product library holds none of it
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert not [l for l in out.splitlines() if "cnrma_recon_" in l]
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "--check recon.resources.txt recon_" in makefile and "libcnrma_recon_hip.so" in makefile.split("\nall:")[1].split("\n")[0]


def test_workspace_query():
    q = recon_lib().cnrma_recon_head_workspace_bytes
    assert q(1, 1, 2, 2, 2) > 0 and q(2, 32, 48, 48, 20) % 16 == 0
    assert q(2, 32, 48, 48, 20) >= 32 * 8 * -(-2 * 48 * 48 * 20 // 512)          # one fp64 partial per wave of 512 voxels and channel
    assert q(1, 1, 96, 96, 40) >= 16 * -(-96 * 96 // (2048 // 40))               # one (sum, count) per workgroup of whole columns
    for bad in ((0, 1, 2, 2, 2), (1, 0, 2, 2, 2), (1, 1, 0, 2, 2), (1, 1, 2, -2, 2), (1, 1, 2, 2, 0), (1, 1, 2048, 2048, 512),
                (2, 1, 1024, 1024, 1024)):
        assert q(*bad) == 0


FWD_ARGS = dict(x=64, elem=0, w=64, prev=64, PX=1, PY=2, PZ=3, threshold=0.99, label_smoothing=1.05, B=1, C=2, X=2, Y=4, Z=6,
                tsdf=64, stream=None)
FWD_BAD = [dict(B=0), dict(C=0), dict(X=3), dict(Y=2), dict(Z=7), dict(PX=2), dict(PZ=0), dict(elem=3), dict(elem=-1), dict(x=None),
           dict(w=None), dict(tsdf=None), dict(prev=None), dict(X=0, PX=0), dict(X=4096, Y=4096, Z=512, PX=2048, PY=2048, PZ=256)]


@pytest.mark.parametrize("bad", FWD_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_forward_refuses_bad_arguments_before_any_launch(bad):
    """every refusal is answered on the host: the pointers are not even device pointers, so a launch would be a fault"""
    lib = recon_lib()
    assert lib.cnrma_recon_head_forward(*dict(FWD_ARGS, **bad).values()) == -22
    assert lib.cnrma_recon_head_forward(*dict(FWD_ARGS, prev=None, PX=0, PY=0, PZ=1).values()) == -22


LOSS_ARGS = dict(tsdf=64, prev=64, PX=1, PY=2, PZ=3, threshold=0.99, trgt=64, B=1, X=2, Y=4, Z=6, workspace=64,
                 workspace_bytes=1 << 20, dloss=None, loss=64, count=64, stream=None)
LOSS_BAD = [dict(B=0), dict(X=4), dict(PY=1), dict(tsdf=None), dict(trgt=None), dict(loss=None), dict(count=None),
            dict(workspace=None), dict(workspace=72), dict(workspace_bytes=8), dict(prev=None)]
BWD_ARGS = dict(x=64, elem=2, w=64, prev=64, PX=1, PY=2, PZ=3, threshold=0.99, label_smoothing=1.05, tsdf=64, grad_tsdf=64,
                dloss=64, grad_loss=64, count=64, B=1, C=2, X=2, Y=4, Z=6, workspace=64, workspace_bytes=1 << 20, dx=64, dw=64,
                stream=None)
BWD_BAD = [dict(C=0), dict(Z=8), dict(elem=5), dict(w=None), dict(tsdf=None), dict(grad_loss=None), dict(count=None),
           dict(workspace=None), dict(workspace_bytes=8), dict(workspace=68), dict(x=None), dict(prev=None)]


@pytest.mark.parametrize("bad", LOSS_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_loss_refuses_bad_arguments_before_any_launch(bad):
    assert recon_lib().cnrma_recon_head_loss_f32(*dict(LOSS_ARGS, **bad).values()) == -22


@pytest.mark.parametrize("bad", BWD_BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_backward_refuses_bad_arguments_before_any_launch(bad):
    lib = recon_lib()
    assert lib.cnrma_recon_head_backward(*dict(BWD_ARGS, **bad).values()) == -22
    assert lib.cnrma_recon_head_backward(*dict(BWD_ARGS, dx=None, dw=None).values()) == 0      # nothing asked for: nothing launched


def test_wrapper_needs_a_gpu_for_cpu_tensors():
    from cnrma_amd import recon
    from cnrma_amd._lib import CnrmaError
    with pytest.raises(CnrmaError, match="GPU|HIP device"):
        recon.tsdf_head_scale(torch.zeros(1, 2, 2, 2, 2), torch.zeros(2), None, 0.99, 1.05)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference(name):
    """float64 restatement against the reference's outputs and losses, each scale on the reference's own previous output:
    near / far, the fill's sign, `use` and its count exactly, values and losses within the parity bound"""
    c = load_case(name)
    for i in range(3):
        prev = c["tsdfs"][i - 1] if i else None
        r = RO.scale(c["xs"][i], c["ws"][i], prev, c["thresholds"][i - 1] if i else 0.0, c["label_smoothing"], c["targets"][i])
        ref = c["tsdfs"][i]
        if i:
            far = ~r["near"]
            assert torch.equal(r["tsdf"][far].float(), ref[far])                             # the fill, sign included: exact
            assert torch.equal(ref[far], (RO.upsample(prev)[far].sign() * 0.999))
        assert float((r["tsdf"] - ref.double()).abs().max()) <= TOL
        use = ((c["targets"][i] < 1) | (c["targets"][i] == 1).all(-1, keepdim=True)) & r["near"]
        assert torch.equal(r["use"], use) and r["count"] == int(use.sum())
        assert same_loss(r["loss"], c["losses"][i]), (name, i, float(r["loss"]), float(c["losses"][i]))
    chained = RO.chain(c["xs"], c["ws"], c["thresholds"], c["label_smoothing"], c["targets"])
    for i, r in enumerate(chained):                                       # ... and handing its own outputs on changes no choice here
        assert float((r["tsdf"] - c["tsdfs"][i].double()).abs().max()) <= TOL and same_loss(r["loss"], c["losses"][i])


def test_fixture_reaches_every_branch():
    c = load_case("mixed")
    far = [~RO.near_mask(c["tsdfs"][i - 1], c["thresholds"][i - 1]) for i in (1, 2)]
    assert all(0.2 < float(f.float().mean()) < 0.9 for f in far)
    assert {float(s) for s in c["tsdfs"][2][far[1]].sign().unique()} == {-1.0, 1.0}
    assert all(bool((t == 1).all(-1).any()) for t in c["targets"])
    c = load_case("allfar")
    assert bool((~RO.near_mask(c["tsdfs"][0], 0.99)).all()) and float(c["losses"][1]) == 0.0 and float(c["losses"][2]) == 0.0
    assert bool(RO.near_mask(load_case("allnear")["tsdfs"][1], 0.99).all())
    assert np.isnan(float(load_case("empty0")["losses"][0]))


def _module(c, impl="torch"):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_head
    channels = [x.shape[1] for x in c["xs"]]
    head = build_head(dict(type="AtlasTSDFHead", input_channels=channels[::-1], n_scales=3, voxel_size=0.04,
                           label_smoothing=c["label_smoothing"], sparse_threshold=c["thresholds"], impl=impl))
    for dec, w in zip(head.decoders, c["ws"]):
        dec.weight.data.copy_(w.reshape(dec.weight.shape))
    return head


@pytest.mark.parametrize("name", CASES)
def test_torch_module_reproduces_the_reference(name):
    """the project's own module (impl="torch", the default): its fill branch and its loss against the reference for the first time"""
    c = load_case(name)
    head = _module(c)
    assert head.impl == "torch"
    with torch.no_grad():
        out, losses = head(c["xs"], {"tsdf_gt_" + k: t for k, t in zip(KEYS, c["targets"])})
    assert list(out) == ["scene_tsdf_" + k for k in KEYS] and list(losses) == ["tsdf_loss_" + k for k in KEYS]
    for i, k in enumerate(KEYS):
        got, ref = out["scene_tsdf_" + k], c["tsdfs"][i]
        if i:
            far = ~RO.near_mask(c["tsdfs"][i - 1], c["thresholds"][i - 1])
            assert torch.equal(got[far], ref[far])
        assert float((got - ref).abs().max()) <= TOL
        assert same_loss(losses["tsdf_loss_" + k], c["losses"][i]), (name, k)
    # the float32 restatement the device tests compare with IS the module's arithmetic
    chained = RO.chain(c["xs"], c["ws"], c["thresholds"], c["label_smoothing"], c["targets"], dtype=torch.float32)
    for r, k in zip(chained, KEYS):
        assert torch.equal(r["tsdf"], out["scene_tsdf_" + k])
        assert torch.equal(torch.as_tensor(r["loss"]), torch.as_tensor(losses["tsdf_loss_" + k])) or np.isnan(float(r["loss"]))


def test_module_keyword():
    c = load_case("allnear")
    assert _module(c, impl="device").impl == "device"
    with pytest.raises(ValueError):
        _module(c, impl="triton")
    assert set(_module(c).state_dict()) == set(_module(c, impl="device").state_dict())
