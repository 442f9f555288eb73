"""Training step (reference app/ml/training/trainer.py): the loss's analytic backward, the validation metrics counted on
the device, and the trainer surface.

Goldens: tests/golden/dbloss_grad.npz (tests/golden/make_golden_loss_grad.py: torch autograd of the reference's own DiceLoss +
nn.BCELoss in float32 and float64, and sklearn's P / R / F1 through the reference's own on_validation_epoch_end).

Gradient bound (GPU): entries where the float64 gradient exceeds 1e3 in magnitude (p in {0, 1} against the other label and its
neighbours: aten's 1e-12 clamp) agree to 1e-6 relative with both goldens.  Everywhere else, per element,
    |hip - g64| <= 2 |g32 - g64| + 4 ulp_fp32(g64)
where g32 is the reference's own float32 autograd: the HIP gradient is no further from the exact value than twice the reference's own
float32 error, plus a few roundings.  (The per-element arithmetic is torch's, in torch's order; only the three sums behind the Dice term
are more exact -- fp64-accumulated -- than torch's fp32 sums.)"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("b2_64x80", "b1_37x53")
SMOOTH = 1e-5


def _recipe():
    spec = importlib.util.spec_from_file_location("make_golden_loss", os.path.join(HERE, "golden", "make_golden_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)      # (only its seeded input recipe is used here)
    return mod.cases()


@pytest.fixture(scope="module")
def grad_golden():
    return np.load(os.path.join(HERE, "golden", "dbloss_grad.npz"))


@pytest.fixture(scope="module")
def inputs():
    stored = np.load(os.path.join(HERE, "golden", "dbloss.npz"))
    cases = _recipe()
    for name in CASES:   # the stored inputs ARE what the recipe regenerates
        for key, t in zip(("prob", "thresh", "prob_t", "thresh_t"), cases[name]):
            assert np.array_equal(stored[f"{name}/{key}"], t.numpy()), (name, key)
    return {name: cases[name] for name in CASES}


def _ref_loss(p, th, pt, tht, weights=None):
    """trainer.py:52-56 restated with torch ops (nn.BCELoss twice + the Dice formula of trainer.py:135-142), for torch autograd."""
    bce = nn.BCELoss()
    prob_loss, thresh_loss = bce(p, pt), bce(th, tht)
    pv, tv = p.reshape(-1), pt.reshape(-1)
    d = 1 - (2. * (pv * tv).sum() + SMOOTH) / (pv.sum() + tv.sum() + SMOOTH)
    if weights is None:
        return prob_loss + thresh_loss + d
    return weights[0] * prob_loss + weights[1] * thresh_loss + weights[2] * d


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------

def test_grad_golden_matches_the_recipe(inputs, grad_golden):
    for name, (prob, *_rest) in inputs.items():
        for w in ("unit", "weighted"):
            for tag in ("32", "64"):
                for key in ("prob", "thresh"):
                    g = grad_golden[f"{name}/{w}/grad_{key}{tag}"]
                    assert g.shape == tuple(prob.shape) and g.dtype == (np.float32 if tag == "32" else np.float64)
    # the golden's float32 gradients are exactly torch's CPU autograd of the restated formulas on the stored inputs
    prob, thresh, prob_t, thresh_t = inputs["b1_37x53"]
    p, th = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    _ref_loss(p, th, prob_t, thresh_t).backward()
    assert np.array_equal(p.grad.numpy(), grad_golden["b1_37x53/unit/grad_prob32"])
    assert np.array_equal(th.grad.numpy(), grad_golden["b1_37x53/unit/grad_thresh32"])


def test_counts_to_precision_recall_f1_match_sklearn(grad_golden):
    from vtd_amd.training import precision_recall_f1
    counts, prf = grad_golden["counts"], grad_golden["prf"]
    assert len(counts) >= 5
    for (tp, fp, fn, _tn), want in zip(counts, prf):
        got = precision_recall_f1(tp, fp, fn)
        assert list(got) == list(want), ((tp, fp, fn), got, want)


def test_trainer_surface_imports_and_hyperparameters():
    from app.ml.training import trainer
    from vtd_amd import training
    for name in ("DiceLoss", "TextDetectionLightningModule", "TextDetectionDataset", "ModelTrainer", "detection_loss"):
        assert getattr(trainer, name) is getattr(training, name)
    model = nn.Conv2d(3, 2, 1)
    m = trainer.TextDetectionLightningModule(model, learning_rate=3e-4, weight_decay=2e-5)
    assert m.forward is not None and m.model is model
    cfg = m.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert isinstance(opt, torch.optim.AdamW) and cfg["lr_scheduler"]["monitor"] == "val_loss"
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["weight_decay"] == 2e-5
    assert {id(p) for p in opt.param_groups[0]["params"]} == {id(p) for p in model.parameters()}
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau)
    assert sched.mode == "min" and sched.factor == 0.5 and sched.patience == 5
    d = trainer.TextDetectionLightningModule(model)
    assert d.learning_rate == 1e-4 and d.weight_decay == 1e-5


def test_model_trainer_is_an_explicit_stub():
    from app.ml.training.trainer import ModelTrainer
    t = ModelTrainer({"max_epochs": 1, "checkpoint_dir": "ckpt", "learning_rate": 1e-4, "weight_decay": 1e-5})
    assert t.config["max_epochs"] == 1 and t.model is None and t.trainer is None
    for call in (lambda: t.setup_trainer(None), lambda: t.train(None, [], []), lambda: t.evaluate(None, [])):
        with pytest.raises(NotImplementedError, match="Trainer"):
            call()


def test_text_detection_dataset():
    from app.ml.training.trainer import TextDetectionDataset
    imgs = [np.full((4, 4, 3), i, np.uint8) for i in range(3)]
    tgts = [{"probability_map": np.zeros((4, 4), np.float32) + i} for i in range(3)]
    ds = TextDetectionDataset(imgs, tgts)
    assert len(ds) == 3 and ds[1][0] is imgs[1] and ds[1][1] is tgts[1]
    ds = TextDetectionDataset(imgs, tgts, transform=lambda im: im.astype(np.float32) * 2)
    im, tg = ds[2]
    assert im.dtype == np.float32 and float(im[0, 0, 0]) == 4.0 and tg is tgts[2]


def test_loss_refuses_targets_that_require_grad_and_models_without_threshold():
    from vtd_amd import training
    p, t = torch.rand(8), torch.rand(8).requires_grad_()
    with pytest.raises(ValueError, match="targets are constants"):
        training.DiceLoss()(p, t)

    class NoThreshold(nn.Module):
        def forward(self, x):
            return {"probability": torch.sigmoid(x[:, :1]), "threshold": None}

    m = training.TextDetectionLightningModule(NoThreshold())
    batch = (torch.zeros(1, 3, 4, 4), {"probability_map": torch.zeros(1, 1, 4, 4), "threshold_map": torch.zeros(1, 1, 4, 4)})
    with pytest.raises(ValueError, match="no threshold map"):
        m.training_step(batch, 0)


def test_metric_counts_without_updates_are_zero():
    from vtd_amd.training import BinaryMetricCounts
    m = BinaryMetricCounts()
    assert m.compute() == {"precision": 0.0, "recall": 0.0, "f1": 0.0}


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_against_golden(got, g32, g64, what):
    got, g32, g64 = got.astype(np.float64).reshape(-1), g32.astype(np.float64).reshape(-1), g64.reshape(-1)
    sat = np.abs(g64) > 1e3
    if sat.any():
        assert np.all(np.abs(got[sat] - g64[sat]) <= 1e-6 * np.abs(g64[sat])), what
        assert np.all(np.abs(got[sat] - g32[sat]) <= 1e-6 * np.abs(g32[sat])), what
    e_hip, e_ref = np.abs(got - g64)[~sat], np.abs(g32 - g64)[~sat]
    bound = 2 * e_ref + 4 * _ulp32(g64[~sat])
    worst = int(np.argmax(e_hip - bound))
    assert np.all(e_hip <= bound), (what, e_hip[worst], e_ref[worst], g64[~sat][worst])
    return int(sat.sum())


@pytest.mark.gpu
def test_hip_gradients_match_the_reference_goldens(hip, inputs, grad_golden):
    from vtd_amd import training
    n_sat = 0
    w = tuple(float(v) for v in grad_golden["weights"])
    for name, (prob, thresh, prob_t, thresh_t) in inputs.items():
        for wname in ("unit", "weighted"):
            p, th = prob.cuda().requires_grad_(), thresh.cuda().requires_grad_()
            r = training.detection_loss({"probability": p, "threshold": th},
                                        {"probability_map": prob_t.cuda(), "threshold_map": thresh_t.cuda()})
            total = r["loss"] if wname == "unit" else w[0] * r["prob_loss"] + w[1] * r["thresh_loss"] + w[2] * r["dice_loss"]
            total.backward()
            for key, got in (("prob", p.grad), ("thresh", th.grad)):
                assert got.dtype == torch.float32 and got.shape == prob.shape
                n_sat += _check_against_golden(got.cpu().numpy(), grad_golden[f"{name}/{wname}/grad_{key}32"],
                                               grad_golden[f"{name}/{wname}/grad_{key}64"], (name, wname, key))
    assert n_sat >= 8     # the saturated entries of b2_64x80 were exercised


@pytest.mark.gpu
def test_dice_loss_carries_a_gradient_and_mixes_with_torch_bce(hip, inputs):
    from vtd_amd import training
    prob, thresh, prob_t, thresh_t = (t.cuda() for t in inputs["b1_37x53"])
    p = prob.clone().requires_grad_()
    d = training.DiceLoss()(p, prob_t)
    assert d.requires_grad and d.grad_fn is not None
    with torch.no_grad():
        d_plain = training.DiceLoss()(p, prob_t)
    assert not d_plain.requires_grad and float(d_plain) == float(d.detach())   # no_grad: the forward of before, same bits

    # the reference's training_step shape: torch's own nn.BCELoss twice + our DiceLoss, against torch autograd of the reference formulas
    p1, th1 = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    bce = nn.BCELoss()
    (bce(p1, prob_t) + bce(th1, thresh_t) + training.DiceLoss()(p1, prob_t)).backward()
    p2, th2 = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    _ref_loss(p2, th2, prob_t, thresh_t).backward()
    n = prob.numel()
    assert torch.equal(th1.grad, th2.grad)                                        # torch's own BCE path, untouched
    assert torch.allclose(p1.grad, p2.grad, rtol=1e-5, atol=1e-5 / n), float((p1.grad - p2.grad).abs().max())
    # the Dice gradient really arrived: without it the two differ by far more than the tolerance
    p3 = prob.clone().requires_grad_()
    bce(p3, prob_t).backward()
    assert float((p1.grad - p3.grad).abs().max()) > 1 / n


@pytest.mark.gpu
def test_half_precision_map_gets_a_half_precision_gradient(hip, inputs):
    from vtd_amd import training
    prob, thresh, prob_t, thresh_t = (t.cuda() for t in inputs["b1_37x53"])
    p16, th16 = prob.half().requires_grad_(), thresh.half().requires_grad_()
    r = training.detection_loss({"probability": p16, "threshold": th16}, {"probability_map": prob_t, "threshold_map": thresh_t})
    r["loss"].backward()
    p32, th32 = p16.detach().float().requires_grad_(), th16.detach().float().requires_grad_()
    training.detection_loss({"probability": p32, "threshold": th32}, {"probability_map": prob_t, "threshold_map": thresh_t})["loss"].backward()
    for g16, g32, src in ((p16.grad, p32.grad, p16), (th16.grad, th32.grad, th16)):
        assert g16.dtype == torch.float16 and g16.shape == src.shape
        assert torch.equal(g16, g32.half())


@pytest.mark.gpu
def test_backward_is_bitwise_repeatable_and_checks_alignment(hip, inputs):
    from vtd_amd import _native, training
    prob, thresh, prob_t, thresh_t = (t.cuda() for t in inputs["b2_64x80"])
    grads = []
    for _ in range(2):
        p, th = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
        training.detection_loss({"probability": p, "threshold": th}, {"probability_map": prob_t, "threshold_map": thresh_t})["loss"].backward()
        grads.append((p.grad, th.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # the 16-byte rule: a map one element into an allocation is refused before any launch
    import ctypes as C
    lib = _native.require()
    buf = torch.zeros(64, device="cuda")
    sums = torch.zeros(5, dtype=torch.float64, device="cuda")
    g = torch.zeros(4, device="cuda")
    out = torch.empty(64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.vtd_dbloss_backward(C.c_void_p(buf.data_ptr() + 4), None, ptr(buf), None, 60, SMOOTH, ptr(sums), ptr(g), ptr(out), None,
                                   None) == -2712
    assert lib.vtd_dbloss_backward(ptr(buf), None, ptr(buf), None, 60, SMOOTH, ptr(sums), ptr(g), None, ptr(out), None) == -2711
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert lib.vtd_binary_counts_accumulate(C.c_void_p(buf.data_ptr() + 4), ptr(buf), 60, 0.5, ptr(counts), None) == -2722
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_backward_at_full_size_matches_torch_gpu_autograd(hip):
    """B = 32 maps of 640 x 640: the HIP gradients against torch's own GPU autograd of the reference formulas."""
    from vtd_amd import training
    g = torch.Generator(device="cuda").manual_seed(11)
    shape = (32, 1, 640, 640)
    prob = torch.sigmoid(torch.randn(shape, generator=g, device="cuda") * 2)
    thresh = torch.sigmoid(torch.randn(shape, generator=g, device="cuda"))
    prob_t = (torch.rand(shape, generator=g, device="cuda") < 0.15).float()
    thresh_t = 0.3 + 0.4 * torch.rand(shape, generator=g, device="cuda")
    n = prob.numel()
    p1, th1 = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    r = training.detection_loss({"probability": p1, "threshold": th1}, {"probability_map": prob_t, "threshold_map": thresh_t})
    r["loss"].backward()
    p2, th2 = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    ref = _ref_loss(p2, th2, prob_t, thresh_t)
    ref.backward()
    assert abs(float(r["loss"].detach()) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    for got, want in ((p1.grad, p2.grad), (th1.grad, th2.grad)):
        err = (got - want).abs()
        assert bool((err <= 1e-5 * want.abs() + 1e-5 / n).all()), float(err.max())


def _np_counts(pred, tgt, thr=0.5):
    pos = pred > thr            # NaN compares False
    one, zero = tgt == 1.0, tgt == 0.0
    return [int((pos & one).sum()), int((pos & zero).sum()), int((~pos & one).sum()), int((~(one | zero)).sum())]


@pytest.mark.gpu
def test_counts_kernel_against_numpy(hip):
    from vtd_amd.training import BinaryMetricCounts
    rng = np.random.default_rng(3)
    for n in (1, 3, 4, 4097, 10007, 2 * 640 * 640 + 3):
        pred = rng.random(n, dtype=np.float32)
        tgt = (rng.random(n) < 0.3).astype(np.float32)
        if n >= 8:
            pred[:4] = [np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0]   # NaN negative, 0.5 not > 0.5
            tgt[4:8] = [np.nan, 0.5, 2.0, -0.0]                                          # three foreign values, -0 is 0
        m = BinaryMetricCounts()
        m.update(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda())
        want = _np_counts(pred, tgt)
        assert list(m.raw_counts()) == want, (n, m.raw_counts(), want)
        if want[3]:
            with pytest.raises(ValueError, match="binary"):
                m.compute()
    # accumulation over a batch split (unequal parts, one not a multiple of 4) equals the whole
    pred = torch.rand(3, 1, 333, 517, device="cuda")
    tgt = (torch.rand(3, 1, 333, 517, device="cuda") < 0.4).float()
    whole, split = BinaryMetricCounts(), BinaryMetricCounts()
    whole.update(pred, tgt)
    flat_p, flat_t = pred.reshape(-1), tgt.reshape(-1)
    cut = 4 * 50001     # 16-byte aligned start of the second part (whose length is not a multiple of 4)
    split.update(flat_p[:cut], flat_t[:cut])
    split.update(flat_p[cut:], flat_t[cut:])
    assert whole.raw_counts() == split.raw_counts() == tuple(_np_counts(pred.cpu().numpy(), tgt.cpu().numpy()))
    split.reset()
    assert split.raw_counts() == (0, 0, 0, 0)


class _TinyDB(nn.Module):
    """A differentiable stand-in for DBNet: {'probability', 'threshold'} maps from two small convolutions."""

    def __init__(self):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 2, 3, padding=1))

    def forward(self, x):
        y = torch.sigmoid(self.body(x))
        return {"probability": y[:, :1], "threshold": y[:, 1:]}


@pytest.mark.gpu
def test_training_step_backward_and_adamw_match_torch(hip):
    import copy
    from vtd_amd import training
    torch.manual_seed(0)
    model = _TinyDB().cuda()
    twin = copy.deepcopy(model)
    g = torch.Generator().manual_seed(1)
    images = torch.randn(2, 3, 48, 40, generator=g).cuda()
    targets = {"probability_map": (torch.rand(2, 1, 48, 40, generator=g) < 0.25).float().cuda(),
               "threshold_map": (0.3 + 0.4 * torch.rand(2, 1, 48, 40, generator=g)).cuda()}

    mod = training.TextDetectionLightningModule(model)
    opt = mod.configure_optimizers()["optimizer"]
    opt.zero_grad()
    loss = mod.training_step((images, targets), 0)
    assert loss.requires_grad
    loss.backward()
    assert set(mod.logged) == {"train_loss", "train_prob_loss", "train_thresh_loss", "train_dice_loss"}
    assert all(v.is_cuda and not v.requires_grad for v in mod.logged.values())

    opt2 = torch.optim.AdamW(twin.parameters(), lr=1e-4, weight_decay=1e-5)
    opt2.zero_grad()
    out = twin(images)
    ref = _ref_loss(out["probability"], out["threshold"], targets["probability_map"], targets["threshold_map"])
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    for (name, a), b in zip(model.named_parameters(), twin.parameters()):
        assert torch.allclose(a.grad, b.grad, rtol=1e-4, atol=1e-6 * float(b.grad.abs().max())), (name, float((a.grad - b.grad).abs().max()))
    opt.step()
    opt2.step()
    for (name, a), b in zip(model.named_parameters(), twin.parameters()):
        assert torch.allclose(a, b, rtol=0, atol=1e-6), (name, float((a - b).abs().max()))


@pytest.mark.gpu
def test_validation_epoch_through_the_product_dbnet(hip):
    from oracle import loss as oloss
    from vtd_amd import nets as mynets
    from vtd_amd import training

    net = mynets.DBNet("resnet18", compute_threshold=True)
    net.load_state_dict(mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5))

    class Recording(nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner, self.seen = inner, []

        def forward(self, x):
            out = self.inner(x)
            self.seen.append({k: v.cpu().numpy() for k, v in out.items()})
            return out

    model = Recording(net)
    mod = training.TextDetectionLightningModule(model)
    g = torch.Generator().manual_seed(2)
    batches = []
    for _ in range(2):
        images = torch.randn(2, 3, 640, 640, generator=g)
        targets = {"probability_map": (torch.rand(2, 1, 640, 640, generator=g) < 0.3).float().cuda(),
                   "threshold_map": (0.3 + 0.4 * torch.rand(2, 1, 640, 640, generator=g)).cuda()}
        batches.append((images, targets))
    with torch.no_grad():
        losses = [float(mod.validation_step(b, i)) for i, b in enumerate(batches)]
    assert len(mod.validation_losses) == 2
    mod.on_validation_epoch_end()
    assert not mod.validation_losses and mod.validation_counts.raw_counts() == (0, 0, 0, 0)

    tp = fp = fn = 0
    for seen, (_, targets) in zip(model.seen, batches):
        c = _np_counts(seen["probability"], targets["probability_map"].cpu().numpy())
        tp, fp, fn = tp + c[0], fp + c[1], fn + c[2]
    assert tp > 0 and fp > 0 and fn > 0
    want_p, want_r = tp / (tp + fp), tp / (tp + fn)
    assert mod.logged["val_precision"] == want_p and mod.logged["val_recall"] == want_r
    assert mod.logged["val_f1"] == 2 * tp / (2 * tp + fp + fn)
    assert float(mod.logged["val_loss"]) == float(torch.tensor(losses).mean())
    ora = [oloss.detection_loss(seen, {k: v.cpu().numpy() for k, v in t.items()})["loss"] for seen, (_, t) in zip(model.seen, batches)]
    assert abs(float(mod.logged["val_loss"]) - np.mean(ora)) <= 1e-5 * np.mean(ora)
