"""Generator of the TSDF-head fixture (not collected by pytest; run in the build container, where the reference is mounted):

    python tests/golden/make_golden_tsdf_head.py            # writes tsdf_head.npz beside this file

It imports the reference's AtlasTSDFHead from where it lies (tests/golden/_ref_import.py), runs it on the CPU WITH targets -- its
only obstacle is a hard `.cuda()` on the loss placeholder (atlas_head.py:58), so torch.Tensor.cuda is the identity while it runs --
and saves inputs, decoder weights, targets, the three outputs and the three losses of every case.  No reference source is copied:
only what its module computes is saved.  The archive is written with a fixed time stamp.

Cases (label_smoothing 1.05, sparse_threshold 0.99 as the shipped configs):
  mixed     B=2, channels 3 / 5 / 8, (2,3,3) -> (4,6,6) -> (8,12,12), decoder weights of std 1.5: no far voxel at the first scale,
            about a third at the second, most at the third, both fill signs; targets hold x-slabs of exact ones (column_all_one)
  allfar    the first scale saturates everywhere: the second and third are filled entirely, their losses are the exact-zero branch
  allnear   small weights: no voxel is ever filled
  empty0    no usable target voxel at the first scale: its loss is the mean of nothing, NaN
The generator asserts and prints that both fill signs occur, that each branch named above is reached, and that the share of voxels
whose parent lies within 1e-4 of the threshold stays under 1 % of every scale (the cap tests/test_recon_gpu.py sets)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402

LABEL_SMOOTHING, THRESHOLDS, KEYS = 1.05, [0.99, 0.99, 0.99], ("016", "008", "004")
MARGIN, CAP = 1e-4, 0.01


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


def run_reference(ah, xs, ws, targets):
    channels = [x.shape[1] for x in xs]
    head = ah.AtlasTSDFHead(input_channels=channels[::-1], n_scales=len(xs), voxel_size=0.04, label_smoothing=LABEL_SMOOTHING,
                            sparse_threshold=THRESHOLDS)
    for dec, w in zip(head.decoders, ws):
        dec.weight.data.copy_(w.reshape(dec.weight.shape))
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            out, losses = head([x.clone() for x in xs], {"tsdf_gt_" + k: t for k, t in zip(KEYS, targets)})
    finally:
        torch.Tensor.cuda = real_cuda
    return [out["scene_tsdf_" + k] for k in KEYS], [torch.as_tensor(losses["tsdf_loss_" + k]).float() for k in KEYS]


def grids(first):
    return [tuple(n * 2 ** i for n in first) for i in range(3)]


def random_targets(gen, B, first, slabs=True):
    """values in (-1, 1), a fifth of them unobserved (exactly 1) inside observed columns, and x-slabs of exact ones"""
    out = []
    for dims in grids(first):
        t = torch.rand(B, 1, *dims, generator=gen) * 2 - 1
        t[torch.rand(B, 1, *dims, generator=gen) < 0.2] = 1.0
        if slabs:
            t[:, :, : max(1, dims[0] // 4)] = 1.0
        out.append(t)
    return out


def make_cases():
    cases = {}
    gen = torch.Generator().manual_seed(20240607)
    # mixed
    B, first, channels = 2, (2, 3, 3), (3, 5, 8)
    xs = [torch.randn(B, c, *d, generator=gen) for c, d in zip(channels, grids(first))]
    ws = [torch.randn(c, generator=gen) * 1.5 for c in channels]
    cases["mixed"] = (xs, ws, random_targets(gen, B, first))
    # allfar: |y| >= 20 at the first scale, both signs
    B, first, channels = 1, (1, 2, 2), (2, 3, 4)
    xs = [torch.randn(B, c, *d, generator=gen) for c, d in zip(channels, grids(first))]
    sign = torch.where(torch.rand(B, *grids(first)[0], generator=gen) < 0.5, -1.0, 1.0)
    xs[0][:, 0] = sign * (0.5 + torch.rand(B, *grids(first)[0], generator=gen))
    ws = [torch.tensor([40.0, 0.0]), torch.randn(3, generator=gen), torch.randn(4, generator=gen)]
    cases["allfar"] = (xs, ws, random_targets(gen, B, first, slabs=False))
    # allnear
    xs = [torch.randn(B, c, *d, generator=gen) for c, d in zip(channels, grids(first))]
    ws = [torch.randn(c, generator=gen) * 0.2 for c in channels]
    cases["allnear"] = (xs, ws, random_targets(gen, B, first))
    # empty0: every first-scale target is 1 except one value above 1 per column -- not observed, and no column is all ones
    xs = [torch.randn(B, c, *d, generator=gen) for c, d in zip(channels, grids(first))]
    ws = [torch.randn(c, generator=gen) * 0.5 for c in channels]
    targets = random_targets(gen, B, first)
    targets[0] = torch.ones_like(targets[0])
    targets[0][..., 0] = 1.5
    cases["empty0"] = (xs, ws, targets)
    return cases


def main():
    _, ah = R.load_reference_atlas3d()
    arrays = dict(label_smoothing=np.float64(LABEL_SMOOTHING), thresholds=np.asarray(THRESHOLDS, np.float64))
    fill_signs, seen = set(), set()
    for name, (xs, ws, targets) in make_cases().items():
        tsdfs, losses = run_reference(ah, xs, ws, targets)
        far_share = []
        for i, (x, w, t, o, l) in enumerate(zip(xs, ws, targets, tsdfs, losses)):
            arrays.update({f"{name}_x{i}": x.numpy(), f"{name}_w{i}": w.numpy(), f"{name}_gt{i}": t.numpy(),
                           f"{name}_tsdf{i}": o.numpy(), f"{name}_loss{i}": l.numpy()})
            assert o.dtype == torch.float32 and l.dtype == torch.float32 and l.dim() == 0
            if i == 0:
                far_share.append(0.0)
                continue
            up = tsdfs[i - 1].repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
            far = ~(up.abs() < THRESHOLDS[i - 1])
            fill_signs.update(np.sign(o[far].numpy()).tolist())
            assert bool((o[far].abs() == np.float32(0.999)).all())
            close = float(((up.abs() - THRESHOLDS[i - 1]).abs() <= MARGIN).float().mean())
            assert close < CAP, (name, i, close)
            far_share.append(float(far.float().mean()))
            print(f"{name} scale {i}: far {far_share[-1]:.3f}, parent within {MARGIN} of the threshold {close:.4f} (cap {CAP})")
        col_one = [(t == 1).all(-1) for t in targets]
        print(f"{name}: losses {[float(l) for l in losses]}, far share {far_share}")
        if name == "mixed":
            assert far_share[0] == 0 and 0.2 < far_share[1] < 0.8 and far_share[2] > far_share[1]
            assert all(bool(c.any()) and not bool(c.all()) for c in col_one)
            seen.add("column_all_one")
        if name == "allfar":
            assert far_share[1] == 1.0 and far_share[2] == 1.0 and float(losses[1]) == 0.0 and float(losses[2]) == 0.0
            assert np.signbit(losses[1].numpy()) == False and torch.isfinite(losses[0])  # noqa: E712
            seen.add("exact zero")
        if name == "allnear":
            assert far_share == [0.0, 0.0, 0.0] and all(torch.isfinite(l) and l > 0 for l in losses)
            seen.add("all near")
        if name == "empty0":
            assert torch.isnan(losses[0]) and torch.isfinite(losses[1]) and torch.isfinite(losses[2])
            seen.add("nan")
    assert fill_signs >= {-1.0, 1.0}, fill_signs
    assert seen == {"column_all_one", "exact zero", "all near", "nan"}, seen
    print("fill signs", sorted(fill_signs), "branches reached", sorted(seen))
    path = os.path.join(HERE, "tsdf_head.npz")
    save_npz(path, arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
