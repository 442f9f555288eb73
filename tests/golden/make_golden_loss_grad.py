"""Generates tests/golden/dbloss_grad.npz from the REFERENCE's own training code.

Needs the reference checkout (make_golden_loss.REF).  The unmodified app/ml/training/trainer.py is exec'd with the same inert
pytorch_lightning stub as make_golden_loss.py, and the inputs are make_golden_loss.cases() (the two small ones: saturated entries, an odd
map size).  Stored:

* torch-autograd gradients of the training step's total (trainer.py:52-56: the reference's DiceLoss instance + nn.BCELoss, verbatim
  order) w.r.t. the probability and threshold maps, in float32 and in float64 (the same float32 inputs widened), for two upstream
  gradients: 1.0 on the total ("unit"), and unequal weights on the three terms ("weighted", WEIGHTS);
* sklearn's binary precision / recall / F1 for a table of {TP, FP, FN, TN} counts, computed by the reference's own
  on_validation_epoch_end (trainer.py:83-105) on prediction / target maps built from those counts.

    python tests/golden/make_golden_loss_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_loss  # noqa: E402

CASES = ("b2_64x80", "b1_37x53")
WEIGHTS = {"unit": None, "weighted": (0.7, 1.9, 2.6)}
# {TP, FP, FN, TN}: empty positives, all-zero targets, all-one targets, no predicted positives, mixed, large
COUNTS = np.array([[0, 0, 0, 10], [0, 3, 0, 7], [5, 0, 2, 0], [0, 0, 4, 6], [37, 11, 5, 100], [123457, 7, 99999, 1]], np.int64)


def grads(tr, prob, thresh, prob_t, thresh_t, dtype, weights):
    p = prob.detach().to(dtype, copy=True).requires_grad_()
    th = thresh.detach().to(dtype, copy=True).requires_grad_()
    pt, tht = prob_t.to(dtype), thresh_t.to(dtype)
    dice_loss, bce_loss = tr.DiceLoss(), torch.nn.BCELoss()
    prob_loss = bce_loss(p, pt)
    thresh_loss = bce_loss(th, tht)
    d = dice_loss(p, pt)
    if weights is None:
        total = prob_loss + thresh_loss + d
    else:
        total = weights[0] * prob_loss + weights[1] * thresh_loss + weights[2] * d
    total.backward()
    return p.grad.numpy(), th.grad.numpy()


def counts_metrics(tr):
    out = []
    for tp, fp, fn, tn in COUNTS:
        pred = torch.tensor([0.9] * (tp + fp) + [0.1] * (fn + tn), dtype=torch.float32)
        tgt = torch.tensor([1.0] * tp + [0.0] * fp + [1.0] * fn + [0.0] * tn, dtype=torch.float32)
        m = tr.TextDetectionLightningModule(torch.nn.Identity())
        logged = {}
        m.log = lambda name, value, **kw: logged.__setitem__(name, value)
        half = len(pred) // 2       # two validation batches
        m.validation_outputs = [{"loss": torch.tensor(1.0), "predictions": pred[:half], "targets": tgt[:half]},
                                {"loss": torch.tensor(1.0), "predictions": pred[half:], "targets": tgt[half:]}]
        m.on_validation_epoch_end()
        out.append([float(logged["val_precision"]), float(logged["val_recall"]), float(logged["val_f1"])])
    return np.array(out, np.float64)


def main():
    tr = make_golden_loss.load_trainer()
    cases = make_golden_loss.cases()
    blob = {"weights": np.array(WEIGHTS["weighted"], np.float64)}
    for name in CASES:
        prob, thresh, prob_t, thresh_t = cases[name]      # stored in dbloss.npz (tests check the recipe against it)
        for wname, w in WEIGHTS.items():
            for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
                gp, gt = grads(tr, prob, thresh, prob_t, thresh_t, dtype, w)
                blob[f"{name}/{wname}/grad_prob{tag}"], blob[f"{name}/{wname}/grad_thresh{tag}"] = gp, gt
            print(name, wname, blob[f"{name}/{wname}/grad_prob32"].reshape(-1)[:4])
    blob["counts"] = COUNTS
    blob["prf"] = counts_metrics(tr)
    print(np.concatenate([COUNTS, blob["prf"]], 1))
    np.savez_compressed(os.path.join(HERE, "dbloss_grad.npz"), **blob)


if __name__ == "__main__":
    main()
