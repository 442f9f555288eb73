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
retained maps.  ReduceLROnPlateau is torch's, as in the reference; the AdamW update is torch's by default and, with
``TextDetectionLightningModule(..., optimizer="hip")``, one multi-tensor HIP pass per parameter group (``AdamW`` below: vtd_adamw_step,
csrc/adamw.hip) behind torch.optim.AdamW's own state and interface.  pytorch_lightning is not part of this build:
``TextDetectionLightningModule`` is a plain ``nn.Module`` with the reference's step methods and ``ModelTrainer`` is a stub.  Like every
other product entry there is no CPU fallback (tensors must live on the GPU, the library must be present).
"""
import ctypes as C
import math

import numpy as np
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


# ---- optimiser (trainer.py:107-112) -------------------------------------------------------------------------------------------------

class AdamW(torch.optim.AdamW):
    """torch.optim.AdamW whose ``step`` is one multi-tensor HIP pass per parameter group (include/vtd.h: vtd_adamw_step): 28 B of HBM
    traffic per element instead of torch's ten or so passes.  Everything but ``step`` is torch's: ``param_groups``, ``state_dict()`` /
    ``load_state_dict()``, schedulers; the per-parameter state is what torch writes (``step`` a CPU float32 scalar, ``exp_avg``,
    ``exp_avg_sq``), so optimiser state dicts move both ways between this class and torch.optim.AdamW; the ``step`` scalars of one
    group's parameters are 0-d views of one CPU vector, so that a step advances them with one add.  Parameters without a gradient
    are skipped and their ``step`` does not move; ``lr`` is read from the group at every step.  float32 arithmetic, every operation
    rounded once (csrc/adamw.hip): the results agree with torch's float32 kernels to rounding, not bit for bit.

    The constructor looks at hyper-parameters only (it can be built around CPU parameters); ``step`` checks the tensors before any
    launch: a parameter with a gradient must be a contiguous float32 CUDA tensor with a dense contiguous float32 gradient on the same
    device -- anything else raises ``_native.NativeError`` (no CPU path).  amsgrad, maximize, capturable, differentiable, fused and a
    tensor ``lr`` are refused, by the constructor and again by every ``step`` (``load_state_dict`` replaces ``param_groups``)."""

    _REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "fused")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable, fused=fused)
        for k in self._REFUSED:
            if given[k]:
                raise ValueError(f"training.AdamW: {k}=True is not built (the HIP step is plain AdamW); use torch.optim.AdamW for it")
        if torch.is_tensor(lr):
            raise ValueError("training.AdamW: a tensor lr is not supported (the step reads lr on the host); pass a float")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=foreach,
                         capturable=False, differentiable=False, fused=None)

    @property
    def _tables(self):
        """group index -> _GroupTable, reused while the group's tensors stay what and where they are.  Not part of the pickled state
        (torch's Optimizer.__getstate__ keeps defaults, state and param_groups): a copy starts with none."""
        return self.__dict__.setdefault("_hip_tables", {})

    def _check_group(self, group):
        for k in self._REFUSED:
            if group.get(k):
                raise ValueError(f"training.AdamW: param_groups carry {k}=True (loaded from another optimiser's state dict?): not built")
        if torch.is_tensor(group["lr"]) or any(torch.is_tensor(b) for b in group["betas"]):
            raise ValueError("training.AdamW: tensor lr / betas are not supported (the step forms its scalars on the host)")

    @staticmethod
    def _check_tensor(t, what, device=None, shape=None):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _native.NativeError(f"training.AdamW: {what} is on {t.device if torch.is_tensor(t) else type(t).__name__}: a CUDA (HIP) "
                                      "tensor is required -- the optimiser step has no CPU path")
        if t.layout != torch.strided or t.dtype != torch.float32 or not t.is_contiguous():
            raise _native.NativeError(f"training.AdamW: {what} must be a dense contiguous float32 tensor (got {t.dtype}, {t.layout}, "
                                      f"contiguous={t.layout == torch.strided and t.is_contiguous()})")
        if device is not None and t.device != device:
            raise _native.NativeError(f"training.AdamW: {what} is on {t.device}, its parameter on {device}")
        if shape is not None and t.shape != shape:
            raise _native.NativeError(f"training.AdamW: {what} has shape {tuple(t.shape)}, its parameter {tuple(shape)}")

    def _build_table(self, gi, live):
        """Full checks of the group's parameters and state (created here on first use, as torch.optim.Adam._init_group writes it), then the
        reused table: p, m, v and n are written once, g and the two per-tensor floats at every step."""
        dev = live[0].device
        entries = []
        for i, p in enumerate(live):
            self._check_tensor(p, f"parameter {i} of group {gi}")
            if p.device != dev:
                raise _native.NativeError(f"training.AdamW: the parameters of group {gi} live on more than one device ({dev}, {p.device})")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            for k in ("exp_avg", "exp_avg_sq"):
                self._check_tensor(st.get(k), f"state {k} of parameter {i} of group {gi}", p.device, p.shape)
            if not torch.is_tensor(st.get("step")) or st["step"].is_cuda or st["step"].dim() != 0:
                raise _native.NativeError(f"training.AdamW: state step of parameter {i} of group {gi} must be a CPU scalar tensor, as "
                                          "torch.optim.AdamW keeps it without capturable / fused")
            entries.append([st, st["exp_avg"], st["exp_avg_sq"], st["step"]])
        # the step counts of the table's parameters move into ONE CPU float32 vector and every state["step"] becomes a 0-d view of its
        # element (still a CPU float32 scalar tensor, as torch keeps it): a step advances them with one add instead of one per parameter
        steps = torch.tensor([float(e[3]) for e in entries], dtype=torch.float32)
        for i, e in enumerate(entries):
            e[0]["step"] = e[3] = steps[i]
        table = (_native.AdamwTensor * len(live))()
        rec = np.frombuffer(table, dtype=_ADAMW_RECORD)   # the same memory, for whole-column writes
        rec["p"] = [p.data_ptr() for p in live]
        rec["m"] = [e[1].data_ptr() for e in entries]
        rec["v"] = [e[2].data_ptr() for e in entries]
        rec["n"] = [p.numel() for p in live]
        t = self._tables[gi] = _GroupTable(tuple(map(id, live)), self.state, entries, rec["p"].tolist(), steps, table, rec, dev)
        return t

    def _refuse(self, gi, group):
        """The slow walk that names what the per-step check tripped over."""
        live = [p for p in group["params"] if p.grad is not None]
        for i, p in enumerate(live):
            self._check_tensor(p, f"parameter {i} of group {gi}")
            self._check_tensor(p.grad, f"the gradient of parameter {i} of group {gi}", p.device, p.shape)
        raise _native.NativeError(f"training.AdamW: group {gi} holds a tensor the HIP step cannot take")

    def _prepare(self, gi, group):
        """Checks one group and returns (table, gradients) without launching anything; None when no parameter has a gradient.  Per step
        and tensor this looks at what can change between steps: the gradient (a new tensor every time: dense and contiguous; its dtype,
        shape and device torch itself holds to the parameter's), the identity of the parameter and of its state tensors and the parameter's
        address.  Everything else was checked when the table was built, and any change of those rebuilds it."""
        self._check_group(group)
        live, grads = [], []
        try:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_contiguous():   # False for sparse COO; the compressed sparse layouts raise
                    self._refuse(gi, group)
                live.append(p)
                grads.append(g)
        except RuntimeError as e:
            if isinstance(e, _native.NativeError):
                raise
            self._refuse(gi, group)
        if not live:
            return None
        t = self._tables.get(gi)
        fresh = t is not None and t.state is self.state and t.ids == tuple(map(id, live))
        if fresh:
            get = self.state.get
            for p, (st, m, v, k), ptr in zip(live, t.entries, t.pptrs):
                if get(p) is not st or st.get("exp_avg") is not m or st.get("exp_avg_sq") is not v or st.get("step") is not k or p.data_ptr() != ptr:
                    fresh = False
                    break
        if not fresh:
            t = self._build_table(gi, live)
        return t, grads

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every group and tensor is checked before the first launch
        work = [(group, w) for group, w in ((group, self._prepare(gi, group)) for gi, group in enumerate(self.param_groups)) if w is not None]
        if not work:
            return loss
        lib = _native.require()
        for group, (t, grads) in work:
            lr, (beta1, beta2) = float(group["lr"]), group["betas"]
            counts = t.steps.add_(1.0).tolist()
            rec = t.rec
            rec["g"] = [g.data_ptr() for g in grads]
            if min(counts) == max(counts):   # the usual case: one step count for the whole group
                k = counts[0]
                rec["step_size"], rec["bc2_sqrt"] = lr / (1.0 - beta1 ** k), math.sqrt(1.0 - beta2 ** k)
            else:
                rec["step_size"] = [lr / (1.0 - beta1 ** k) for k in counts]
                rec["bc2_sqrt"] = [math.sqrt(1.0 - beta2 ** k) for k in counts]
            hyper = _native.AdamwHyper(1.0 - lr * float(group["weight_decay"]), 1.0 - beta1, beta2, 1.0 - beta2, float(group["eps"]))
            with torch.cuda.device(t.device):
                _native.check(lib.vtd_adamw_step(t.table, len(grads), C.byref(hyper), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                              "vtd_adamw_step")
        return loss


# vtd_adamw_tensor as a numpy record, to write a column of the table at once
_ADAMW_RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert _ADAMW_RECORD.itemsize == C.sizeof(_native.AdamwTensor) == 48


class _GroupTable:
    """One parameter group's reused vtd_adamw_tensor table and what it was built from (identities of the parameters, of the state dict
    and of its tensors, the parameters' addresses): any change rebuilds it."""
    __slots__ = ("ids", "state", "entries", "pptrs", "steps", "table", "rec", "device")

    def __init__(self, *values):
        for k, v in zip(self.__slots__, values):
            setattr(self, k, v)


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

    OPTIMIZERS = ("torch", "hip")

    def __init__(self, model: nn.Module, learning_rate: float = 1e-4, weight_decay: float = 1e-5, optimizer: str = "torch"):
        super().__init__()
        if optimizer not in self.OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {self.OPTIMIZERS} (got {optimizer!r}): 'torch' is torch.optim.AdamW as in the "
                             "reference, 'hip' the same update as one HIP pass per parameter group (training.AdamW)")
        self.optimizer = optimizer
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
        cls = AdamW if self.optimizer == "hip" else torch.optim.AdamW
        optimizer = cls(self.parameters(), lr=self.learning_rate, weight_decay=self.weight_decay)
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
