"""The fused training node (sparse.conv_bn_act_train) against the composition it stands for (conv_autograd, then batch_norm_train),
and MinkowskiConvolution's differentiable fused epilogue against the same thing in torch: the same kernels in the same order, so
every output, gradient and running statistic is exact.  Small shapes: ~300 voxels, and the 2 voxels the fused rule starts at."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BN_TRAIN = ("cnrma_bn_train_forward_f32", "cnrma_bn_train_backward_f32")


def _voxels(n_vox):
    """int32 [n, 4] (batch, x, y, z): two neighbours on the x axis that a stride of 2 keeps apart, or ~300 of a 10^3 cube"""
    if n_vox == 2:
        return np.array([[0, 1, 0, 0], [0, 2, 0, 0]], dtype=np.int32)
    rng = np.random.RandomState(11)
    c = np.concatenate((np.zeros((340, 1), dtype=np.int64), rng.randint(-5, 5, size=(340, 3))), axis=1)
    return np.unique(c, axis=0).astype(np.int32)


def _tensor(S, device, c, f):
    return S.SparseTensor(torch.from_numpy(f).to(device).requires_grad_(True), S.CoordSet(torch.from_numpy(c).to(device), 1))


def _bn(cout, device):
    rng = np.random.RandomState(cout)
    bn = torch.nn.BatchNorm1d(cout).to(device).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.randn(cout).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.randn(cout).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, cout).astype(np.float32)))
    return bn


def _recorded(S, fn):
    """fn() with S.call recording the entry-point names -> (result, names)"""
    names, orig = [], S.call
    S.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    try:
        return fn(), names
    finally:
        S.call = orig


CASES = [(act, res, 3, 1, 32, 32) for act in (None, "relu", "elu") for res in (False, True)] + \
        [("relu", True, 1, 1, 32, 64), ("relu", True, 3, 2, 32, 64)]
REFUSED = [("relu", False, 3, 1, 32, 260), ("relu", False, 3, 1, 32, 34)]       # C > 256; C % 4 != 0: BatchNorm through torch


@pytest.mark.parametrize("n_vox", [300, 2])
@pytest.mark.parametrize("act,with_res,k,s,cin,cout", CASES + REFUSED)
def test_fused_node_equals_conv_then_batch_norm(device, act, with_res, k, s, cin, cout, n_vox):
    from cnrma_amd import sparse as S
    c = _voxels(n_vox)
    rng = np.random.RandomState(k * 100 + s * 10 + cout)
    f = rng.randn(len(c), cin).astype(np.float32)
    W = (rng.randn(*((k ** 3, cin, cout) if k > 1 else (cin, cout))) / np.sqrt(cin * k ** 3)).astype(np.float32)
    bn0 = _bn(cout, device)
    got = {}
    for fused in (True, False):
        bn = copy.deepcopy(bn0)
        x = _tensor(S, device, c, f)
        Wd = torch.from_numpy(W).to(device).requires_grad_(True)
        out_cs = x.cs if s == 1 else x.cs.strided(s)
        assert out_cs.n >= 2
        res = None
        if with_res:
            rf = torch.from_numpy(np.random.RandomState(4).randn(out_cs.n, cout).astype(np.float32)).to(device)
            res = S.SparseTensor(rf.requires_grad_(True), out_cs)

        def run():
            if fused:
                y = S.conv_bn_act_train(x, Wd, bn, k, s, act, res).F
            else:
                y = S.batch_norm_train(S.conv_autograd(x, Wd, k, s).F, bn, act or False, None if res is None else res.F)
            y.backward(torch.from_numpy(np.random.RandomState(1).randn(*y.shape).astype(np.float32)).to(device))
            return y

        y, names = _recorded(S, run)
        assert y.shape == (out_cs.n, cout)
        want = 0 if (cout > 256 or cout % 4) else 1          # what the library's BatchNorm accepts runs on it exactly once
        assert [names.count(n) for n in BN_TRAIN] == [want, want], names
        grads = [x.F.grad, Wd.grad, bn.weight.grad, bn.bias.grad] + ([res.F.grad] if with_res else [])
        assert all(g is not None for g in grads)
        got[fused] = [t.detach().cpu().numpy() for t in [y] + grads + [bn.running_mean, bn.running_var, bn.num_batches_tracked]]
    assert int(got[True][-1]) == 1 and not np.array_equal(got[True][-3], bn0.running_mean.cpu().numpy())
    for a, e in zip(got[True], got[False]):
        np.testing.assert_array_equal(a, e)


def test_convolution_module_differentiable_epilogue_equals_torch_composition(device):
    """MinkowskiConvolution.forward with scale, shift, residual and act while gradients are wanted (the fused kernel has no
    backward) against conv_autograd followed by the same torch operations written out here"""
    from cnrma_amd import nn as snn, sparse as S
    c = _voxels(300)
    rng = np.random.RandomState(2)
    f = rng.randn(len(c), 32).astype(np.float32)
    torch.manual_seed(5)
    conv = snn.MinkowskiConvolution(32, 32, kernel_size=3, stride=2, dimension=3).to(device)
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, 32).astype(np.float32)).to(device)
    shift = torch.from_numpy(rng.randn(32).astype(np.float32)).to(device)
    got = {}
    for module in (True, False):
        conv.kernel.grad = None
        x = _tensor(S, device, c, f)
        out_cs = x.cs.strided(2)
        res = S.SparseTensor(torch.from_numpy(np.random.RandomState(4).randn(out_cs.n, 32).astype(np.float32)).to(device), out_cs)
        if module:
            y = conv(x, scale=scale, shift=shift, residual=res, act="elu")
            assert y.cs is out_cs
            y = y.F
        else:
            y = S.conv_autograd(x, conv.kernel, 3, 2).F
            y = torch.nn.functional.elu(y * scale.view(1, -1) + shift.view(1, -1) + res.F)
        y.backward(torch.from_numpy(np.random.RandomState(1).randn(*y.shape).astype(np.float32)).to(device))
        got[module] = [t.detach().cpu().numpy() for t in (y, x.F.grad, conv.kernel.grad)]
    assert np.abs(got[True][1]).max() > 0 and np.abs(got[True][2]).max() > 0
    for a, e in zip(got[True], got[False]):
        np.testing.assert_array_equal(a, e)
