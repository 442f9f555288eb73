"""Training-side surface of the reference (app/ml/training/trainer.py): the loss of its training / validation step with an analytic
backward, the validation metrics, and the Lightning module's step methods.

``DiceLoss`` has the reference's constructor and ``forward(pred, target)`` (trainer.py:130-142); ``detection_loss(outputs, targets)``
is the four-scalar body of ``TextDetectionLightningModule.training_step`` / ``validation_step`` (trainer.py:48-56, 66-71):

    prob_loss   = nn.BCELoss()(outputs['probability'], targets['probability_map'])
    thresh_loss = nn.BCELoss()(outputs['threshold'],   targets['threshold_map'])
    dice_loss   = DiceLoss()(outputs['probability'],   targets['probability_map'])
    total_loss  = prob_loss + thresh_loss + dice_loss

Both run as ONE HBM-bound HIP pass over the maps (include/vtd.h: vtd_dbloss_forward; csrc/dbloss.hip).  When a map requires grad, the
scalars are views of one autograd node whose backward is one element-wise HIP pass (vtd_dbloss_backward) that forms what torch autograd
forms on the reference's graph; targets are constants (a target that requires grad is refused -- torch's BCELoss would differentiate it,
no caller of the reference does).  The validation metrics are three integer counts per batch (vtd_binary_counts_accumulate), not the
retained maps.  AdamW and ReduceLROnPlateau are torch's, as in the reference.  pytorch_lightning is not part of this build:
``TextDetectionLightningModule`` is a plain ``nn.Module`` with the reference's step methods and ``ModelTrainer`` is a stub.  Like every
other product entry there is no CPU fallback (tensors must live on the GPU, the library must be present).
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.utils.data import Dataset

from . import _native


def _f32_cuda(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _native.NativeError(f"{name}: a CUDA (HIP) tensor is required -- the loss has no CPU path")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _run(prob, thresh, prob_t, thresh_t, smooth, want_sums=False):
    lib = _native.require()
    prob, prob_t = _f32_cuda(prob, "pred"), _f32_cuda(prob_t, "target")
    if prob.numel() != prob_t.numel() or prob.numel() == 0:
        raise ValueError(f"pred and target must have the same, non-zero number of elements ({prob.numel()} vs {prob_t.numel()})")
    if (thresh is None) != (thresh_t is None):
        raise ValueError("threshold map and threshold target come together")
    if thresh is not None:
        thresh, thresh_t = _f32_cuda(thresh, "threshold"), _f32_cuda(thresh_t, "threshold target")
        if thresh.numel() != prob.numel() or thresh_t.numel() != prob.numel():
            raise ValueError("threshold maps must have the probability map's element count")
    ws = torch.empty(int(lib.vtd_dbloss_workspace_bytes()), dtype=torch.uint8, device=prob.device)
    out = torch.empty(4, dtype=torch.float32, device=prob.device)
    sums = torch.empty(5, dtype=torch.float64, device=prob.device) if want_sums else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _native.check(lib.vtd_dbloss_forward(ptr(prob), ptr(thresh), ptr(prob_t), ptr(thresh_t), prob.numel(), float(smooth), ptr(ws), ptr(out),
                                         ptr(sums), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_dbloss_forward")
    return out, sums


def _check_targets(*targets):
    for t in targets:
        if torch.is_tensor(t) and t.requires_grad:
            raise ValueError("loss targets are constants: a target that requires grad is not supported (detach it); the reference's "
                             "callers never differentiate their targets")


class _DetectionLossFn(torch.autograd.Function):
    """float32[4] {prob BCE, thresh BCE, dice, total} of vtd_dbloss_forward; backward: vtd_dbloss_backward with the [4] upstream gradient
    as it arrives (read on the device) and the forward's fp64 sums."""

    @staticmethod
    def forward(ctx, smooth, prob, thresh, prob_t, thresh_t):
        ctx.smooth = smooth
        ctx.in_meta = [(t.shape, t.dtype) if t is not None else None for t in (prob, thresh)]
        ctx.has_thresh = thresh is not None
        names = ("pred", "threshold", "target", "threshold target")
        f32 = [_f32_cuda(t, nm) if t is not None else None for t, nm in zip((prob, thresh, prob_t, thresh_t), names)]   # cast once
        out, sums = _run(*f32, smooth, want_sums=True)
        ctx.save_for_backward(sums, *[t for t in f32 if t is not None])
        ctx.mark_non_differentiable(sums)
        return out, sums

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_sums):
        lib = _native.require()
        sums, *maps = ctx.saved_tensors
        if ctx.has_thresh:
            prob, thresh, prob_t, thresh_t = maps
        else:
            (prob, prob_t), thresh, thresh_t = maps, None, None
        want_p, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_thresh
        if grad_out is None:
            grad_out = torch.zeros(4, dtype=torch.float32, device=prob.device)
        g = grad_out.to(device=prob.device, dtype=torch.float32).contiguous()
        gp = torch.empty_like(prob) if want_p else None
        gt = torch.empty_like(prob) if want_t else None
        if gp is None and gt is None:
            return None, None, None, None, None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _native.check(lib.vtd_dbloss_backward(ptr(prob), ptr(thresh), ptr(prob_t), ptr(thresh_t), prob.numel(), float(ctx.smooth), ptr(sums),
                                              ptr(g), ptr(gp), ptr(gt), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                      "vtd_dbloss_backward")
        (sp, dp), tmeta = ctx.in_meta[0], ctx.in_meta[1]
        gp = gp.view(sp).to(dp) if gp is not None else None
        gt = gt.view(tmeta[0]).to(tmeta[1]) if gt is not None else None
        return None, gp, gt, None, None


def _loss(prob, thresh, prob_t, thresh_t, smooth, want_sums=False):
    """(out4, sums5 or None): through the autograd node when grad is enabled and a map requires it, else the plain pass of before."""
    _check_targets(prob_t, thresh_t)
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (prob, thresh)):
        out, sums = _DetectionLossFn.apply(smooth, prob, thresh, prob_t, thresh_t)
        return out, (sums if want_sums else None)
    return _run(prob, thresh, prob_t, thresh_t, smooth, want_sums)


class DiceLoss(nn.Module):
    """trainer.py:130-142: ``1 - (2 sum(pred * target) + smooth) / (sum(pred) + sum(target) + smooth)`` over the flattened maps."""

    def __init__(self, smooth: float = 1e-5):
        super(DiceLoss, self).__init__()
        self.smooth = smooth

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        out, _ = _loss(pred, None, target, None, self.smooth)
        return out[2]


def detection_loss(outputs, targets, smooth: float = 1e-5, want_sums: bool = False):
    """The body of training_step / validation_step (trainer.py:48-56): {'loss', 'prob_loss', 'thresh_loss', 'dice_loss'} as 0-d float32
    tensors on the device (one pass over the four maps, one 16-byte result), differentiable w.r.t. the maps that require grad.
    ``outputs`` is DBNet's output dict ({'probability', 'threshold'}), ``targets`` the batch's {'probability_map', 'threshold_map'}."""
    out, sums = _loss(outputs["probability"], outputs["threshold"], targets["probability_map"], targets["threshold_map"], smooth, want_sums)
    res = {"prob_loss": out[0], "thresh_loss": out[1], "dice_loss": out[2], "loss": out[3]}
    if want_sums:
        res["sums"] = sums
    return res


# ---- validation metrics (trainer.py:83-103) ----------------------------------------------------------------------------------------

def precision_recall_f1(tp, fp, fn):
    """sklearn precision_recall_fscore_support(average='binary', zero_division=0) from the counts: P = TP / (TP + FP),
    R = TP / (TP + FN), F1 = 2 TP / (2 TP + FP + FN), each 0.0 when its denominator is 0 (exact integers, one rounding each)."""
    tp, fp, fn = int(tp), int(fp), int(fn)
    div = lambda a, b: a / b if b else 0.0
    return div(tp, tp + fp), div(tp, tp + fn), div(2 * tp, 2 * tp + fp + fn)


class BinaryMetricCounts:
    """Validation precision / recall / F1 of ``pred > 0.5`` against a {0, 1} target map, accumulated on the device as int64
    {TP, FP, FN, targets not in {0, 1}}: ``update`` never syncs, ``compute`` copies 32 bytes once.  A target outside {0, 1} (NaN included)
    raises ValueError at ``compute``, as sklearn does for non-binary targets -- with one corner: sklearn accepts a target map of one
    foreign value when every prediction is 1 (two labels) and returns zeros; this raises."""

    THRESHOLD = 0.5   # trainer.py:92

    def __init__(self):
        self.counts = None

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()

    def update(self, pred, target):
        lib = _native.require()
        pred, target = _f32_cuda(pred, "pred"), _f32_cuda(target, "target")
        if pred.numel() != target.numel() or pred.numel() == 0:
            raise ValueError(f"pred and target must have the same, non-zero number of elements ({pred.numel()} vs {target.numel()})")
        if self.counts is None or self.counts.device != pred.device:
            self.counts = torch.zeros(4, dtype=torch.int64, device=pred.device)
        _native.check(lib.vtd_binary_counts_accumulate(C.c_void_p(pred.data_ptr()), C.c_void_p(target.data_ptr()), pred.numel(),
                                                       float(self.THRESHOLD), C.c_void_p(self.counts.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_binary_counts_accumulate")

    def raw_counts(self):
        """(TP, FP, FN, foreign) as Python ints (one device-to-host copy)."""
        if self.counts is None:
            return 0, 0, 0, 0
        return tuple(int(v) for v in self.counts.cpu().tolist())

    def compute(self):
        tp, fp, fn, foreign = self.raw_counts()
        if foreign:
            raise ValueError(f"validation targets must be binary: {foreign} target values are not in {{0, 1}}")
        p, r, f1 = precision_recall_f1(tp, fp, fn)
        return {"precision": p, "recall": r, "f1": f1}


# ---- trainer surface (trainer.py:14-30, 32-128, 144-219) ---------------------------------------------------------------------------

class TextDetectionDataset(Dataset):
    """trainer.py:14-30: (image, target) pairs, ``transform`` applied to the image."""

    def __init__(self, images, targets, transform=None):
        self.images = images
        self.targets = targets
        self.transform = transform

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        image = self.images[idx]
        target = self.targets[idx]
        if self.transform:
            image = self.transform(image)
        return image, target


class TextDetectionLightningModule(nn.Module):
    """trainer.py:32-128 without pytorch_lightning: a plain ``nn.Module`` with the reference's constructor and step methods.  ``model``
    returns {'probability', 'threshold'} (DBNet(compute_threshold=True) for validation; training needs a differentiable model -- the
    product DBNet runs forward-only on the HIP engine).  ``log`` keeps the latest value per name in ``self.logged`` (device tensors
    detached, no sync per step).  Validation keeps the per-batch loss scalars and device counts, never the maps."""

    def __init__(self, model: nn.Module, learning_rate: float = 1e-4, weight_decay: float = 1e-5):
        super().__init__()
        self.model = model
        self.learning_rate = learning_rate
        self.weight_decay = weight_decay
        self.dice_loss = DiceLoss()
        self.validation_losses = []
        self.validation_counts = BinaryMetricCounts()
        self.logged = {}

    def forward(self, x):
        return self.model(x)

    def log(self, name, value, **kwargs):
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def _loss(self, batch):
        images, targets = batch
        outputs = self(images)
        if outputs.get("threshold") is None:
            raise ValueError("the model returned no threshold map: the training loss needs both maps (construct DBNet with "
                             "compute_threshold=True)")
        dev = outputs["probability"].device
        targets = {k: targets[k].to(dev, non_blocking=True) for k in ("probability_map", "threshold_map")}
        return outputs, targets, detection_loss(outputs, targets, self.dice_loss.smooth)

    def training_step(self, batch, batch_idx):
        outputs, _, loss = self._loss(batch)
        if torch.is_grad_enabled() and not loss["loss"].requires_grad:
            raise RuntimeError("training_step needs a differentiable model: its maps carry no gradient (the product DBNet runs "
                               "forward-only on the HIP engine)")
        self.log("train_loss", loss["loss"], on_step=True, on_epoch=True, prog_bar=True)
        self.log("train_prob_loss", loss["prob_loss"], on_epoch=True)
        self.log("train_thresh_loss", loss["thresh_loss"], on_epoch=True)
        self.log("train_dice_loss", loss["dice_loss"], on_epoch=True)
        return loss["loss"]

    def validation_step(self, batch, batch_idx):
        outputs, targets, loss = self._loss(batch)
        total = loss["loss"].detach()
        self.validation_losses.append(total)
        self.validation_counts.update(outputs["probability"], targets["probability_map"])
        return total

    def on_validation_epoch_end(self):
        if not self.validation_losses:
            return
        avg_loss = torch.stack(self.validation_losses).mean()
        try:
            m = self.validation_counts.compute()
        finally:
            self.validation_losses.clear()
            self.validation_counts.reset()
        self.log("val_loss", avg_loss, prog_bar=True)
        self.log("val_precision", m["precision"])
        self.log("val_recall", m["recall"])
        self.log("val_f1", m["f1"])

    def configure_optimizers(self):
        optimizer = torch.optim.AdamW(self.parameters(), lr=self.learning_rate, weight_decay=self.weight_decay)
        # the reference also passes verbose=True, which torch 2.10 no longer accepts
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=5)
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "monitor": "val_loss"}}


class ModelTrainer:
    """trainer.py:144-219, constructor only: fitting, checkpointing (ModelCheckpoint top-3 on val_loss), early stopping and test runs
    are pytorch_lightning's Trainer machinery, which this build does not provide."""

    _MISSING = ("needs pytorch_lightning's Trainer with its ModelCheckpoint / EarlyStopping / LearningRateMonitor callbacks, which this "
                "build does not provide; drive TextDetectionLightningModule's training_step / validation_step / on_validation_epoch_end "
                "and configure_optimizers from a loop of your own")

    def __init__(self, config):
        self.config = config
        self.model = None
        self.trainer = None

    def setup_trainer(self, model):
        raise NotImplementedError("ModelTrainer.setup_trainer " + self._MISSING)

    def train(self, model, train_loader, val_loader):
        raise NotImplementedError("ModelTrainer.train " + self._MISSING)

    def evaluate(self, model, test_loader):
        raise NotImplementedError("ModelTrainer.evaluate " + self._MISSING)
