"""Generates tests/golden/dbhead_train.npz from the REFERENCE's own DBHead (app/ml/models/text_detector.py:58-86) in train mode.

Needs the reference checkout (make_golden.REF), loaded under make_golden's import stubs.  The reference's DBHead(256).train() gets
make_golden-style seeded parameters (nets.seeded_state_dict: torch's init under a fixed seed plus non-trivial BatchNorm statistics) and
an fp16-representable [2,256,12,10] input; torch autograd in float32 runs one forward, the training loss (BCE + BCE + Dice, trainer.py:
52-56, on seeded random targets) and its backward.  Stored: the two maps, the loss, the running statistics after the forward, the full
gradients of every small parameter, a seeded sample of the two conv 3x3 weight gradients plus their norms.

    python tests/golden/make_golden_dbhead_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPE = (2, 256, 12, 10)
SEED = 31
N_SAMPLE = 4096


def inputs():
    from vtd_amd import nets
    g = torch.Generator().manual_seed(SEED)
    x = (torch.randn(SHAPE, generator=g) * 0.5).half().float()
    n, _, H, W = SHAPE
    pt = (torch.rand((n, 1, 4 * H, 4 * W), generator=g) > 0.7).float()
    tt = torch.rand((n, 1, 4 * H, 4 * W), generator=g) * 0.6 + 0.2
    sd = nets.seeded_state_dict(lambda: nets.DBHead(256), SEED)
    return x, pt, tt, sd


def sample_index(numel):
    return np.random.default_rng(SEED).choice(numel, N_SAMPLE, replace=False)


def main():
    _, det, _ = make_golden.load_reference()
    x, pt, tt, sd = inputs()
    head = det.DBHead(256)
    head.load_state_dict(sd)
    head.train()
    out = head(x)
    bce = torch.nn.BCELoss()
    p, t = out["probability"], out["threshold"]
    pv, tv = p.view(-1), pt.view(-1)
    dice = 1 - (2.0 * (pv * tv).sum() + 1e-5) / (pv.sum() + tv.sum() + 1e-5)
    loss = bce(p, pt) + bce(t, tt) + dice
    loss.backward()
    rec = {"probability": p.detach().numpy(), "threshold": t.detach().numpy(), "loss": np.float64(loss.item())}
    for k, v in head.state_dict().items():
        if "running" in k:
            rec["after." + k] = v.numpy()
    for k, prm in head.named_parameters():
        g = prm.grad.detach().double().numpy()
        if g.size > 100000:
            rec["grad_sample." + k] = g.reshape(-1)[sample_index(g.size)]
            rec["grad_norm." + k] = np.float64(np.linalg.norm(g))
        else:
            rec["grad." + k] = g
    np.savez_compressed(os.path.join(HERE, "dbhead_train.npz"), **rec)


if __name__ == "__main__":
    main()
