"""GPU parity of the small-footprint halo convolution (csrc/conv_halo.hip: conv_halo_small_kernel, candidate 108: 8 x 16 pixel
blocks x 64 output channels, three workgroups per CU), pinned with VTD_FORCE_HALO=4 wherever it is supported.

The checks and their bounds are the detector's existing ones: every stored tap against the fp64 reference of its own stage
(test_gpu_detector_stages: oracle/stage_bounds.py, sb.T_STAGE), and with seeded default-init weights the taps within 1.5e-2 of
the tap's magnitude and max|dp| <= 2e-3 against the fp32 oracle and against the implicit-GEMM path.  The kernel accumulates
chunk-major, so it is NOT bit-identical to conv_igemm; what must be bit-identical is a second forward on the same engine:
a zero-ring pixel or a neighbouring block written by mistake changes what the next forward reads."""
import numpy as np
import pytest
import torch

from oracle import nets as onets
from vtd_amd import nets as mynets

import test_gpu_detector_stages as stages
from test_gpu_detector import _rel

pytestmark = pytest.mark.gpu

OPTIONS = {"fuse_fpn_head": 0}
TAPS = ("c2", "c3", "c4", "c5", "p2")


def _force(monkeypatch, mode):
    monkeypatch.setenv("VTD_FORCE_HALO", mode)
    monkeypatch.setenv("VTD_HALO_CONV", "0" if mode == "0" else "1")


def _forward_twice(eng, x, n):
    """(probability, taps, launch names) of the first forward; asserts that a second forward repeats it bit for bit."""
    from vtd_amd.engine import detector_profile
    runs = []
    for _ in range(2):
        prob = eng.forward(x)["probability"].cpu().numpy()
        runs.append((prob, {t: eng.read_tap(t, n) for t in TAPS}))
    assert np.array_equal(runs[0][0], runs[1][0]), "probability differs between two forwards on one engine"
    for t in TAPS:
        assert np.array_equal(runs[0][1][t], runs[1][1][t]), f"tap {t} differs between two forwards on one engine"
    return runs[0][0], runs[0][1], [r[0] for r in detector_profile(eng)]


# ResNet-18 at 640 x 640: layer 1 (160 x 160, 64 -> 64, four launches) and the three stride-1 launches of layer 2 (80 x 80: K = 1152
# twice, and K = 1216 for layer2.0 conv2 with the folded downsample as a second K segment) are whole 8 x 16 blocks; layer 3 / 4
# (40 x 40, 20 x 20) are not and stay where they were.  B = 3 gives grids that are no
# multiple of 8 for the XCD re-deal.  ResNet-50: the 3x3 of res2 (160 x 160, 64 -> 64) and of res3's stride-1 blocks (80 x 80).
@pytest.mark.parametrize("backbone,n,at_least", [("resnet18", 1, 7), ("resnet18", 3, 7), ("resnet50", 2, 4)])
def test_stages_with_small_halo_kernel_forced(hip, monkeypatch, backbone, n, at_least):
    from vtd_amd.engine import DetectorEngine
    _force(monkeypatch, "4")
    sd, _ = stages._stress(backbone)
    x = stages._frames(n, 700 if backbone == "resnet18" else 800)
    eng = DetectorEngine(backbone, sd, max_batch=n, options=dict(OPTIONS))
    try:
        prob, taps, kernels = _forward_twice(eng, x, n)
        taps["probability"] = prob
        for t in ("input", "pool", "head1"):
            taps[t] = eng.read_tap(t, n)
    finally:
        eng.close()
    small = [k for k in kernels if "conv_halo_small" in k]
    print(f"[{backbone} B={n}] conv_halo_small launches: {small}")
    assert len(small) >= at_least, kernels
    if backbone == "resnet18":
        assert sum("N=128 K=1152" in k for k in small) == 2 and sum("N=128 K=1216" in k for k in small) == 1, kernels
    stages._check_all(f"{backbone} halo small B={n}", backbone, taps)


@pytest.mark.parametrize("n", [1, 3])
def test_small_halo_kernel_against_oracle_and_implicit_gemm(hip, monkeypatch, n):
    from vtd_amd.engine import DetectorEngine
    sd = mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5)
    x = torch.randn(n, 3, 640, 640, generator=torch.Generator().manual_seed(21))
    ref = onets.dbnet_forward(x, sd, "resnet18", return_taps=True)
    outs = {}
    for mode in ("4", "0"):
        _force(monkeypatch, mode)
        eng = DetectorEngine("resnet18", sd, max_batch=n, options=dict(OPTIONS))
        try:
            outs[mode] = _forward_twice(eng, x, n)
        finally:
            eng.close()
    prob, taps, names = outs["4"]
    errs = {t: _rel(taps[t], ref["taps"][i].numpy()) for i, t in enumerate(("c2", "c3", "c4", "c5"))}
    errs["p2"] = _rel(taps["p2"], ref["p2"].numpy())
    dp = float(np.abs(prob - ref["probability"].numpy()).max())
    d_paths = float(np.abs(prob - outs["0"][0]).max())
    print(f"B={n} tap errors {errs} max|dp| {dp} vs implicit-GEMM path {d_paths} small launches {sum('conv_halo_small' in k for k in names)}")
    assert sum("conv_halo_small" in k and "K=1152" in k for k in names) == 2 and sum("conv_halo_small" in k and "K=1216" in k for k in names) == 1, names
    assert not any("conv_halo" in k for k in outs["0"][2])
    assert all(v < 1.5e-2 for v in errs.values()), errs
    assert dp <= 2e-3 and d_paths <= 2e-3
