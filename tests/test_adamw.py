"""The HIP AdamW step without a device: vtd_adamw_step in the header, the library and the binding table with its two structs, every
refusal of the C entry (all of them return before a launch, so host pointers serve), the refusals of vtd_amd.training.AdamW's constructor
and of its step(), the trainer module's optimizer= switch, and the numpy restatement the GPU tests compare bits against
(vtd_amd/_fixtures/adamw.py) held to torch: its error against torch.optim.AdamW run in float64 may be at most 3x that of torch's own
float32 run of the same gradients."""
import ctypes as C
import math
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from vtd_amd import _native, training
from vtd_amd._fixtures import adamw as fx

ROOT = pathlib.Path(__file__).resolve().parents[1]
ERR = -3601


# ---- C ABI
def _header_int(name):
    m = re.search(rf"#define\s+{name}\s+(\d+)", (ROOT / "include" / "vtd.h").read_text())
    assert m, name
    return int(m.group(1))


def test_header_library_and_binding_agree():
    lib = _native.load()
    header = (ROOT / "include" / "vtd.h").read_text()
    assert "vtd_adamw_step(" in header and "vtd_adamw_step" in _native.SIGNATURES and hasattr(lib, "vtd_adamw_step")
    assert b"AdamW" in lib.vtd_strerror(ERR)
    assert C.sizeof(_native.AdamwTensor) == 48
    assert [(n, C.sizeof(t)) for n, t in _native.AdamwTensor._fields_] == [("p", 8), ("g", 8), ("m", 8), ("v", 8), ("n", 8), ("step_size", 4),
                                                                           ("bc2_sqrt", 4)]
    assert C.sizeof(_native.AdamwHyper) == 20
    assert [n for n, _ in _native.AdamwHyper._fields_] == ["decay", "one_minus_beta1", "beta2", "one_minus_beta2", "eps"]
    # the header's struct members, in order
    body = re.search(r"typedef struct vtd_adamw_tensor \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in _native.AdamwTensor._fields_]
    body = re.search(r"typedef struct vtd_adamw_hyper \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == [n for n, _ in _native.AdamwHyper._fields_]
    assert _header_int("VTD_ADAMW_SLICE") == _native.ADAMW_SLICE == 64
    assert _header_int("VTD_ADAMW_CHUNK") == _native.ADAMW_CHUNK and _native.ADAMW_CHUNK % 1024 == 0
    # 64 entries, the int64 prefix of their chunk counts and the scalars fit HIP's 4 KB of kernel arguments
    assert 64 * 48 + 65 * 8 + 20 + 4 <= 4096


def test_refusals_before_any_launch():
    lib = _native.load()
    step = lib.vtd_adamw_step
    raw = (C.c_float * 64)()
    a = C.addressof(raw)
    a += -a % 16
    hyper = _native.AdamwHyper(1.0, 0.1, 0.999, 0.001, 1e-8)
    hp = C.byref(hyper)

    def table(count=1, **kw):
        t = (_native.AdamwTensor * max(count, 1))()
        for e in t:
            e.p, e.g, e.m, e.v, e.n, e.step_size, e.bc2_sqrt = a, a + 16, a + 32, a + 48, 4, 1e-3, 0.03
        for k, val in kw.items():
            setattr(t[count - 1], k, val)      # the LAST entry is the bad one: the whole table is checked before the first launch
        return t

    assert step(None, 0, None, None) == 0 and step(table(), 0, hp, None) == 0           # count == 0: nothing to do
    assert step(table(), -1, hp, None) == ERR
    assert step(None, 1, hp, None) == ERR and step(table(), 1, None, None) == ERR
    for count in (1, 3, 65, 130):
        for field in ("p", "g", "m", "v"):
            assert step(table(count, **{field: None}), count, hp, None) == ERR, (count, field)
            for off in (1, 2, 3):
                assert step(table(count, **{field: a + off}), count, hp, None) == ERR, (count, field, off)
        for n in (-1, 1 << 40, 1 << 62):
            assert step(table(count, n=n), count, hp, None) == ERR, (count, n)
        for bad in (0.0, -0.5, math.nan, math.inf, -math.inf):
            assert step(table(count, bc2_sqrt=bad), count, hp, None) == ERR, (count, bad)
        for bad in (math.nan, math.inf):
            assert step(table(count, step_size=bad), count, hp, None) == ERR, (count, bad)
    for field, _ in _native.AdamwHyper._fields_:
        for bad in (math.nan, math.inf, -math.inf):
            h = _native.AdamwHyper(1.0, 0.1, 0.999, 0.001, 1e-8)
            setattr(h, field, bad)
            assert step(table(), 1, C.byref(h), None) == ERR, (field, bad)
    # a table of nothing but empty tensors is no work: their pointers are not looked at, nothing is launched
    empty = table(3)
    for e in empty:
        e.p = e.g = e.m = e.v = None
        e.n = 0
    assert step(empty, 3, hp, None) == 0


# ---- vtd_amd.training.AdamW
def test_constructor_checks_hyper_parameters_only():
    conv = nn.Conv2d(3, 4, 3)
    for flag in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        with pytest.raises(ValueError, match=flag):
            training.AdamW(conv.parameters(), **{flag: True})
    with pytest.raises(ValueError, match="tensor lr"):
        training.AdamW(conv.parameters(), lr=torch.tensor(1e-3))
    opt = training.AdamW(conv.parameters(), lr=2e-4, weight_decay=1e-5)      # CPU parameters: fine until step()
    assert isinstance(opt, torch.optim.AdamW)
    g = opt.param_groups[0]
    assert g["lr"] == 2e-4 and g["weight_decay"] == 1e-5 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert not any(g[k] for k in ("amsgrad", "maximize", "capturable", "differentiable", "fused"))
    assert opt.step() is None                                               # no gradients: nothing to check, nothing to launch
    assert len(opt.state) == 0
    for p in conv.parameters():
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in conv.parameters()]
    with pytest.raises(_native.NativeError, match="cpu"):
        opt.step()
    assert len(opt.state) == 0 and all(torch.equal(a, b) for a, b in zip(before, conv.parameters()))


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_step_refuses_flags_that_arrive_through_load_state_dict(flag):
    conv, twin = nn.Conv2d(3, 4, 3), nn.Conv2d(3, 4, 3)
    other = torch.optim.AdamW(twin.parameters(), **{flag: True})
    opt = training.AdamW(conv.parameters())
    opt.load_state_dict(other.state_dict())
    assert opt.param_groups[0][flag] is True
    for p in conv.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match=flag):
        opt.step()


def test_state_dicts_load_in_both_directions():
    """torch.optim.AdamW state (after CPU steps) loads into training.AdamW and comes back out unchanged: same keys, same step type."""
    conv, twin = nn.Conv2d(3, 4, 3), nn.Conv2d(3, 4, 3)
    other = torch.optim.AdamW(twin.parameters(), lr=3e-4, weight_decay=1e-5)
    for p in twin.parameters():
        p.grad = torch.ones_like(p)
    other.step()
    other.step()
    opt = training.AdamW(conv.parameters())
    opt.load_state_dict(other.state_dict())
    sd, want = opt.state_dict(), other.state_dict()
    assert sd["param_groups"] == want["param_groups"]
    for k, st in want["state"].items():
        assert sorted(sd["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        assert sd["state"][k]["step"].dtype == torch.float32 and sd["state"][k]["step"].device.type == "cpu" and float(sd["state"][k]["step"]) == 2.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][k][name], st[name])
    back = torch.optim.AdamW(nn.Conv2d(3, 4, 3).parameters())
    back.load_state_dict(sd)
    assert back.state_dict()["param_groups"] == want["param_groups"]


def test_trainer_module_optimizer_switch():
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
    default = training.TextDetectionLightningModule(model, learning_rate=3e-4, weight_decay=2e-5)
    cfg0 = default.configure_optimizers()
    assert type(cfg0["optimizer"]) is torch.optim.AdamW
    assert type(training.TextDetectionLightningModule(model, optimizer="torch").configure_optimizers()["optimizer"]) is torch.optim.AdamW
    mod = training.TextDetectionLightningModule(model, learning_rate=3e-4, weight_decay=2e-5, optimizer="hip")
    cfg = mod.configure_optimizers()
    opt = cfg["optimizer"]
    assert type(opt) is training.AdamW and isinstance(opt, torch.optim.AdamW)
    g, g0 = opt.param_groups[0], cfg0["optimizer"].param_groups[0]
    assert len(opt.param_groups) == 1 and g["lr"] == 3e-4 and g["weight_decay"] == 2e-5
    assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in g0.items() if k != "params"}
    assert [id(p) for p in g["params"]] == [id(p) for p in mod.parameters()] == [id(p) for p in g0["params"]]
    s, s0 = cfg["lr_scheduler"]["scheduler"], cfg0["lr_scheduler"]["scheduler"]
    assert cfg["lr_scheduler"]["monitor"] == cfg0["lr_scheduler"]["monitor"] == "val_loss"
    assert isinstance(s, torch.optim.lr_scheduler.ReduceLROnPlateau) and s.optimizer is opt
    assert (s.mode, s.factor, s.patience) == (s0.mode, s0.factor, s0.patience) == ("min", 0.5, 5)
    for bad in ("HIP", "sgd", "", None):
        with pytest.raises(ValueError, match="optimizer"):
            training.TextDetectionLightningModule(model, optimizer=bad)
    from app.ml.training import trainer
    assert trainer.AdamW is training.AdamW


# ---- the restatement against torch
STEPS, N, LR, WD = 10, 300_007, 1e-4, 1e-5


def _torch_run(p0, grads, dtype):
    p = torch.tensor(p0, dtype=dtype).requires_grad_()
    opt = torch.optim.AdamW([p], lr=LR, weight_decay=WD, foreach=False)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    st = opt.state[p]
    assert float(st["step"]) == len(grads)
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_is_as_close_to_float64_adamw_as_torch_float32(seed):
    p0, grads = fx.adamw_case(N, STEPS, seed)
    assert np.isfinite(grads).all() and (grads[:, ::97] == 0).all() and np.abs(grads).max() > 10
    sq = grads.astype(np.float64) ** 2
    assert ((sq > 0) & (sq < 2.0 ** -126)).any() and ((sq > 0) & (sq < 2.0 ** -149)).any()      # subnormal squares, and squares below them
    exact = _torch_run(p0, grads, torch.float64)
    ref32 = _torch_run(p0, grads, torch.float32)
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for k, g in enumerate(grads):
        p, m, v = fx.adamw_step_f32(p, g, m, v, k + 1, LR, (0.9, 0.999), 1e-8, WD)
    got, want = fx.adamw_levels((p, m, v), exact, grads, LR), fx.adamw_levels(ref32, exact, grads, LR)
    print(f"seed {seed}: restatement levels {got}, torch float32 levels {want}")
    for k in ("p", "m", "v"):
        assert np.isfinite(want[k]) and want[k] > 0
        assert got[k] <= 3.0 * want[k], (k, got[k], want[k])
    assert (m[::97] == 0).all() and (v[::97] == 0).all()      # an element that never saw a gradient keeps exact zeros
