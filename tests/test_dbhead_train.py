"""DB head training without a device: the fp64 reference the GPU tests use (nets.DBHead's sub-Sequentials under CPU autograd) against the
reference's own DBHead (tests/golden/dbhead_train.npz, make_golden_dbhead_train.py), negative controls of that reference, and the API
refusals that need no device."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import nets

HERE = os.path.dirname(os.path.abspath(__file__))
# the GPU tests' bounds (tests/test_gpu_dbhead_train.py)
BOUNDS = {"small_train": {"grad": 1.5e-3, "map": 1.3e-3, "stat": 6e-5}, "tiny_train": {"grad": 1.2e-3, "map": 9e-4, "stat": 3e-4}}
MOMENTUM = 0.1


def _recipe():
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    spec = importlib.util.spec_from_file_location("make_golden_dbhead_train", os.path.join(HERE, "golden", "make_golden_dbhead_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _loss(p, t, pt, tt):
    bce = torch.nn.BCELoss()
    pv, tv = p.reshape(-1), pt.reshape(-1)
    dice = 1 - (2.0 * (pv * tv).sum() + 1e-5) / (pv.sum() + tv.sum() + 1e-5)
    return bce(p, pt) + bce(t, tt) + dice


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_fp64_reference_reproduces_the_reference_golden():
    rec = _recipe()
    g = np.load(os.path.join(HERE, "golden", "dbhead_train.npz"))
    x, pt, tt, sd = rec.inputs()
    head = nets.DBHead(256)
    head.load_state_dict(sd)
    head = head.double().train()
    p, t = head.probability_head(x.double()), head.threshold_head(x.double())
    loss = _loss(p, t, pt.double(), tt.double())
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert float(np.abs(p.detach().numpy() - g["probability"]).max()) <= 1e-5
    assert float(np.abs(t.detach().numpy() - g["threshold"]).max()) <= 1e-5
    for k, v in head.state_dict().items():
        if "running" in k:
            assert _rel(v.numpy(), g["after." + k]) <= 1e-5, k
    for k, prm in head.named_parameters():
        gr = prm.grad.numpy()
        if k.endswith(("0.bias", "3.bias")):   # in front of a train-mode BatchNorm: exactly zero, both sides are rounding noise
            assert np.abs(gr).max() <= 1e-6 and np.abs(g["grad." + k]).max() <= 1e-6, k
        elif "grad_sample." + k in g:
            assert _rel(gr.reshape(-1)[rec.sample_index(gr.size)], g["grad_sample." + k]) <= 1e-3, k
            assert abs(np.linalg.norm(gr) / float(g["grad_norm." + k]) - 1) <= 1e-4, k
        else:
            assert _rel(gr, g["grad." + k]) <= 1e-3, k


# ---- negative controls: the same bounds must reject a reference with an injected bug by >= 10x
def _functional_branch(seq, x, bug=None):
    """One branch with torch functionals on seq's tensors; `bug` injects a kernel-style mistake."""
    def bn(mod, v):
        dims = (0, 2, 3)
        mean, var_b = v.mean(dims), v.var(dims, unbiased=False)
        n = v.numel() // v.shape[1]
        with torch.no_grad():
            rv = var_b if bug == "biased_running_var" else var_b * n / (n - 1)
            mod.running_mean.mul_(0.9).add_(0.1 * mean)
            mod.running_var.mul_(0.9).add_(0.1 * rv)
        if bug == "bn_no_batch_terms":   # the eval-mode backward in train mode: statistics treated as constants
            mean, var_b = mean.detach(), var_b.detach()
        return (v - mean.view(1, -1, 1, 1)) / torch.sqrt(var_b.view(1, -1, 1, 1) + mod.eps) * mod.weight.view(1, -1, 1, 1) + mod.bias.view(1, -1, 1, 1)

    w0 = seq[0].weight.flip(-1) if bug == "flipped_tap" else seq[0].weight
    y = F.conv2d(x, w0, seq[0].bias, padding=1)
    a = torch.relu(bn(seq[1], y))
    w3 = seq[3].weight.transpose(-1, -2) if bug == "convt_transposed" else seq[3].weight
    z = F.conv_transpose2d(a, w3, seq[3].bias, stride=2)
    a2 = torch.relu(bn(seq[4], z))
    return torch.sigmoid(F.conv_transpose2d(a2, seq[6].weight, seq[6].bias, stride=2))


def _run(bug, shape, xscale=0.5):
    gen = torch.Generator().manual_seed(4)
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 8))
    head = head.double().train()
    before = {k: v.clone() for k, v in head.state_dict().items() if "running" in k}
    n, _, H, W = shape
    x = (torch.randn(shape, generator=gen) * xscale).half().double()
    pt = (torch.rand((n, 1, 4 * H, 4 * W), generator=gen) > 0.7).double()
    tt = torch.rand((n, 1, 4 * H, 4 * W), generator=gen).double() * 0.6 + 0.2
    p = _functional_branch(head.probability_head, x, bug)
    t = _functional_branch(head.threshold_head, x, bug)
    _loss(p, t, pt, tt).backward()
    grads = {k: v.grad.clone() for k, v in head.named_parameters()}
    # the batch statistic each running-stat update implies, as the GPU tests compare it
    stats = {k: (v - (1 - MOMENTUM) * before[k]) / MOMENTUM for k, v in head.state_dict().items() if "running" in k}
    return p.detach(), grads, stats


def test_functional_reference_matches_the_module_reference():
    shape = (2, 256, 6, 5)
    p, grads, stats = _run(None, shape)
    gen = torch.Generator().manual_seed(4)
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 8))
    head = head.double().train()
    before = {k: v.clone() for k, v in head.state_dict().items() if "running" in k}
    x = (torch.randn(shape, generator=gen) * 0.5).half().double()
    pt = (torch.rand((2, 1, 24, 20), generator=gen) > 0.7).double()
    tt = torch.rand((2, 1, 24, 20), generator=gen).double() * 0.6 + 0.2
    pm = head.probability_head(x)
    _loss(pm, head.threshold_head(x), pt, tt).backward()
    assert float((pm - p).abs().max()) <= 1e-12
    for k, v in head.named_parameters():
        if k.endswith(("0.bias", "3.bias")):   # rounding noise on both sides (see above)
            assert float(v.grad.abs().max()) <= 1e-12 and float(grads[k].abs().max()) <= 1e-12, k
        else:
            assert _rel(v.grad.numpy(), grads[k].numpy()) <= 1e-9, k
    for k, v in head.state_dict().items():
        if "running" in k:
            assert _rel(((v - (1 - MOMENTUM) * before[k]) / MOMENTUM).numpy(), stats[k].numpy()) <= 1e-12, k


# shapes and input scale of the GPU parity tests' cases
GPU_CASES = {"small_train": (2, 256, 24, 20), "tiny_train": (2, 256, 4, 3)}


@pytest.mark.parametrize("bug,case,measure", [
    ("bn_no_batch_terms", "small_train", "grad"),
    ("convt_transposed", "small_train", "map"),
    ("flipped_tap", "small_train", "map"),
    ("bn_no_batch_terms", "tiny_train", "grad"),
    ("convt_transposed", "tiny_train", "map"),
    ("flipped_tap", "tiny_train", "map"),
    ("biased_running_var", "small_train", "stat"),
    ("biased_running_var", "tiny_train", "stat"),
])
def test_negative_controls_are_rejected_by_ten_times_the_bound(bug, case, measure):
    shape, bound = GPU_CASES[case], BOUNDS[case][measure]
    p0, g0, s0 = _run(None, shape)
    p1, g1, s1 = _run(bug, shape)
    if measure == "map":
        err = float((p1 - p0).abs().max())
    elif measure == "grad":
        err = max(_rel(g1[k].numpy(), g0[k].numpy()) for k in g0 if k.endswith("0.weight"))
    else:
        err = max(_rel(s1[k].numpy(), s0[k].numpy()) for k in s0)
    assert err >= 10 * bound, f"{bug}: error {err:.3g} is not 10x the bound {bound}"


# ---- refusals that need no device
def test_trainable_values_and_frozen_trunk():
    with pytest.raises(ValueError, match="trainable"):
        nets.DBNet("resnet18", trainable="all")
    net = nets.DBNet("resnet18", compute_threshold=True, trainable="head")
    assert not any(p.requires_grad for p in list(net.backbone.parameters()) + list(net.fpn.parameters()))
    assert all(p.requires_grad for p in net.head.parameters())
    plain = nets.DBNet("resnet18")
    assert plain.trainable is None and all(p.requires_grad for p in plain.backbone.parameters())
    assert plain.set_trainable("head") is plain and plain.trainable == "head"
    with pytest.raises(ValueError):
        plain.set_trainable("fpn")


def test_head_refuses_features_that_require_grad():
    head = nets.DBHead(256)
    with pytest.raises(RuntimeError, match="dgrad into P2"):
        head(torch.zeros((1, 256, 4, 4), requires_grad=True))
    with pytest.raises(ValueError):
        head(torch.zeros((1, 128, 4, 4)))
    # padded features whose extent does not match H, W (or the dtype / layout the kernels read) never reach the device
    for feats, hw in ((torch.zeros((1, 6, 6, 256), dtype=torch.float16), (4, 4)), (torch.zeros((1, 6, 6, 256)), (4, 4)),
                      (torch.zeros((1, 6, 5, 256), dtype=torch.float16), (4, 4)), (torch.zeros((1, 6, 6, 128), dtype=torch.float16), (4, 4))):
        with pytest.raises(ValueError, match="padded features"):
            head.forward_padded(feats, *hw)
