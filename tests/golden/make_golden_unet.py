"""Generator of the wide 3D U-Net fixture (not collected by pytest; run in the build container, where the reference is mounted):

    python tests/golden/make_golden_unet.py                # writes atlas3d_wide.npz beside this file

It imports the reference's AtlasBackbone3D from where it lies (tests/golden/_ref_import.py), builds it at widths the device
convolutions support (tests/unet_fixture.py: channels 32 / 64 / 128, one block per level, norm 'BN'), with cond_proj False and True,
fills its parameters by key (unet_fixture.fill), and runs it in eval mode on unet_fixture.make_input() in fp32 and -- the same module,
converted -- in fp64.  Saved: the input, the fp32 outputs of both cases, and per output the reference's own fp32 error against its
fp64 run (helpers.elementwise_error), the yardstick for what a 1e-4 criterion leaves to another implementation.  No weights are
stored and no reference source is copied.  The archive is written with a fixed time stamp."""
import copy
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_import as R  # noqa: E402
import helpers  # noqa: E402
import unet_fixture as UF  # noqa: E402


def save_npz(path, arrays):
    """np.load-compatible compressed archive with a fixed time stamp (np.savez_compressed stamps the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(arrays[key], requirements="C"), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    b3, _ = R.load_reference_atlas3d()
    x = UF.make_input()
    out = {"x": x.numpy()}
    for tag, cond in UF.CASES:
        net = UF.fill(b3.AtlasBackbone3D(cond_proj=cond, **UF.NET)).eval()
        net64 = copy.deepcopy(net).double().eval()
        with torch.no_grad():
            feats, feats64 = net(x), net64(x.double())
        for i, (f, f64) in enumerate(zip(feats, feats64)):
            out[f"{tag}_feat{i}"] = f.numpy()
            out[f"{tag}_fp32_error{i}"] = np.float64(helpers.elementwise_error(f.numpy(), f64.numpy()))
            print(tag, i, tuple(f.shape), "max|f|", float(f.abs().max()), "fp32 vs fp64", float(out[f"{tag}_fp32_error{i}"]))
            assert out[f"{tag}_fp32_error{i}"] <= 1e-5               # more than 10x below the 1e-4 criterion
    path = os.path.join(HERE, "atlas3d_wide.npz")
    save_npz(path, out)
    print("atlas3d_wide.npz written,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
