"""The HIP AdamW step on the device (csrc/adamw.hip, vtd_amd.training.AdamW): bit equality with the numpy float32 restatement of
vtd_amd/_fixtures/adamw.py (which tests/test_adamw.py holds to torch) at every size where the kernel takes another path -- below, at and
past a chunk, n % 4 tails, tensors that are not 16-byte aligned, more than one and more than two slices of 64 tensors --, a parameter whose
gradient goes missing, two parameter groups under a plateau scheduler, non-finite gradients, optimiser state moving to and from
torch.optim.AdamW, and two end-to-end training rounds of the detector."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from vtd_amd import _native, nets, training
from vtd_amd._fixtures import adamw as fx

pytestmark = pytest.mark.gpu

CHUNK = _native.ADAMW_CHUNK
GUARD = 8                      # floats between neighbouring tensors of an arena (and a multiple of 4: slots stay 16-byte aligned)
GUARD_VALUE = -12345.678
BETAS, EPS = (0.9, 0.999), 1e-8
KINDS = ("p", "g", "m", "v")


def _primes(count, start=7):
    out, k = [], start
    while len(out) < count:
        if all(k % d for d in range(2, int(k ** 0.5) + 1)):
            out.append(k)
        k += 1
    return out


class Arenas:
    """Four device buffers (p, g, m, v), every tensor a view into them with GUARD_VALUE floats on both sides; ``offs[kind][i]`` shifts
    tensor i of that buffer off its 16-byte slot by that many floats."""

    def __init__(self, sizes, offs=None):
        self.sizes = list(sizes)
        offs = offs or {}
        self.spans, self.dev = {}, {}
        for kind in KINDS:
            cursor, spans = GUARD, []
            for i, n in enumerate(self.sizes):
                start = cursor + offs.get(kind, {}).get(i, 0)
                spans.append((start, start + n))
                cursor = (start + n + GUARD + 3) // 4 * 4
            self.spans[kind] = spans
            self.dev[kind] = torch.full((cursor,), GUARD_VALUE, dtype=torch.float32, device="cuda")
            assert self.dev[kind].data_ptr() % 16 == 0

    def image(self, kind, tensors):
        """The host image of an arena holding ``tensors`` (float32 arrays), guards included."""
        a = np.full(self.dev[kind].numel(), GUARD_VALUE, dtype=np.float32)
        for (s, e), t in zip(self.spans[kind], tensors):
            a[s:e] = t
        return a

    def upload(self, kind, tensors):
        self.dev[kind].copy_(torch.from_numpy(self.image(kind, tensors)))

    def views(self, kind):
        return [self.dev[kind][s:e] for s, e in self.spans[kind]]

    def assert_bits(self, kind, tensors, what):
        got, want = self.dev[kind].cpu().numpy().view(np.int32), self.image(kind, tensors).view(np.int32)
        bad = np.flatnonzero(got != want)
        if bad.size:
            owner = [i for i, (s, e) in enumerate(self.spans[kind]) if s - GUARD <= bad[0] < e + GUARD]
            raise AssertionError(f"{what}: {bad.size} words of the {kind} arena differ, first at {bad[0]} (tensor {owner}, span "
                                 f"{self.spans[kind][owner[0]] if owner else None}, n {self.sizes[owner[0]] if owner else None})")


def _case(sizes, steps, seed):
    p0, grads = fx.adamw_case(sum(sizes), steps, seed)
    cuts = np.cumsum(sizes)[:-1]
    return np.split(p0, cuts), [np.split(g, cuts) for g in grads]


def _drive(sizes, offs, steps, seed, group_of=None, groups=({"lr": 1e-4, "weight_decay": 1e-5},), missing=None, halve_after=None):
    """Runs training.AdamW over guarded views for ``steps`` steps and checks all four arenas bit for bit against the restatement after
    every step.  ``missing``: {tensor index: set of 1-based steps at which its grad is None}; ``halve_after``: the step after which a
    plateau scheduler halves every group's lr.  Returns (optimizer, parameters)."""
    ar = Arenas(sizes, offs)
    p, grads = _case(sizes, steps, seed)
    m, v = [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]
    ar.upload("p", p)
    ar.upload("m", m)
    ar.upload("v", v)
    params = [t.requires_grad_() for t in ar.views("p")]
    gviews, mviews, vviews = ar.views("g"), ar.views("m"), ar.views("v")
    group_of = group_of or [0] * len(sizes)
    opt = training.AdamW([dict(params=[q for q, gi in zip(params, group_of) if gi == k], **g) for k, g in enumerate(groups)])
    for q, mv, vv in zip(params, mviews, vviews):   # torch's state layout, with the moments inside the guarded arenas
        opt.state[q] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": mv, "exp_avg_sq": vv}
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0) if halve_after else None
    lrs = [g["lr"] for g in groups]
    count = [0] * len(sizes)
    missing = missing or {}
    for step in range(1, steps + 1):
        ar.upload("g", grads[step - 1])
        for i, q in enumerate(params):
            q.grad = None if step in missing.get(i, ()) else gviews[i]
        opt.step()
        for i in range(len(sizes)):
            if step in missing.get(i, ()):
                continue
            count[i] += 1
            g = groups[group_of[i]]
            p[i], m[i], v[i] = fx.adamw_step_f32(p[i], grads[step - 1][i], m[i], v[i], count[i], lrs[group_of[i]], BETAS, EPS, g["weight_decay"])
        for kind, want in (("p", p), ("m", m), ("v", v), ("g", grads[step - 1])):
            ar.assert_bits(kind, want, f"step {step}")
        assert [float(opt.state[q]["step"]) for q in params] == [float(c) for c in count]
        if sched is not None:
            # a validation loss that improves at every epoch but `halve_after`
            sched.step(2.0 if step == halve_after else (1.0 if step < halve_after else 0.1) / step)
            if step == halve_after:
                lrs = [lr * 0.5 for lr in lrs]
            assert [g["lr"] for g in opt.param_groups] == lrs, (step, lrs)
    return opt, params


SIZES = [1, 3, 4, 5, 255, 1024, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7] + _primes(120)
SHORT_VIEW, LONG_VIEW, LAGGING = 3, 9, 7      # n = 5: p alone starts mid-row; n = 2 CHUNK + 7: all four do; n = CHUNK loses its gradient twice


def test_bit_equal_to_the_restatement_over_six_steps(hip):
    assert len(SIZES) == 130 > 2 * _native.ADAMW_SLICE and SIZES[LONG_VIEW] > CHUNK
    offs = {"p": {SHORT_VIEW: 1, LONG_VIEW: 1}, "g": {LONG_VIEW: 1}, "m": {LONG_VIEW: 1}, "v": {LONG_VIEW: 1}}
    opt, params = _drive(SIZES, offs, 6, seed=11, missing={LAGGING: {2, 3}})
    assert params[SHORT_VIEW].data_ptr() % 16 == 4 and params[LONG_VIEW].data_ptr() % 16 == 4 and params[LAGGING].data_ptr() % 16 == 0
    steps = [float(opt.state[q]["step"]) for q in params]
    assert steps[LAGGING] == 4.0 and all(s == 6.0 for i, s in enumerate(steps) if i != LAGGING)      # it lags by two
    st = opt.state[params[0]]["step"]
    assert st.dtype == torch.float32 and st.device.type == "cpu" and st.dim() == 0


def test_two_groups_under_a_plateau_scheduler(hip):
    """Different lr and weight_decay per group, one with weight_decay = 0 (decay == 1: p * 1 is exact), lr halved between steps 3 and 4."""
    sizes = [CHUNK + 9, 37, 1000, 513, 2 * CHUNK, 11]
    _drive(sizes, None, 5, seed=12, group_of=[0, 0, 0, 1, 1, 1], groups=({"lr": 1e-4, "weight_decay": 1e-5}, {"lr": 3e-3, "weight_decay": 0.0}),
           halve_after=3)


@pytest.mark.parametrize("count", [1, 64, 65])
def test_count_edges_with_the_optimisers_own_state(hip, count):
    """One tensor, exactly one slice, one slice and one tensor; the moments are the optimiser's own zeros, created on first use."""
    sizes = _primes(count, start=5)
    p, grads = _case(sizes, 2, seed=13 + count)
    params = [torch.from_numpy(a).cuda().requires_grad_() for a in p]
    opt = training.AdamW(params, lr=2e-4, weight_decay=1e-2)
    m, v = [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]
    for step in (1, 2):
        for q, g in zip(params, grads[step - 1]):
            q.grad = torch.from_numpy(g).cuda()
        opt.step()
        for i in range(count):
            p[i], m[i], v[i] = fx.adamw_step_f32(p[i], grads[step - 1][i], m[i], v[i], step, 2e-4, BETAS, EPS, 1e-2)
    assert len(opt.state) == count
    for i, q in enumerate(params):
        st = opt.state[q]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 2.0
        for got, want in ((q.detach(), p[i]), (st["exp_avg"], m[i]), (st["exp_avg_sq"], v[i])):
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (i, sizes[i])


def test_non_finite_gradients_stay_where_they_are(hip):
    n = CHUNK + 5
    p0, grads = fx.adamw_case(n, 1, seed=14)
    g = grads[0].copy()
    g[::97] = 1e-3                                     # every element sees a gradient
    nan_at, inf_at = [2, CHUNK - 1, CHUNK + 4], [0, 1023, CHUNK]
    g[nan_at], g[inf_at] = np.nan, np.inf
    g[inf_at[1]] = -np.inf
    q = torch.from_numpy(p0).cuda().requires_grad_()
    opt = training.AdamW([q], lr=1e-4, weight_decay=1e-5)
    q.grad = torch.from_numpy(g).cuda()
    opt.step()
    want = np.zeros(n, bool)
    want[nan_at + inf_at] = True
    for name, t in (("p", q.detach()), ("m", opt.state[q]["exp_avg"]), ("v", opt.state[q]["exp_avg_sq"])):
        assert np.array_equal(~np.isfinite(t.cpu().numpy()), want), name


# ---- state interchange with torch.optim.AdamW
IC_SIZES, IC_LR, IC_WD = (CHUNK + 3, 37, 1000), 1e-4, 1e-5


@pytest.fixture(scope="module")
def interchange_case():
    """Five steps of gradients, torch.optim.AdamW's float64 run of them and the error levels of its float32 run (the 3x yardstick)."""
    p0, grads = _case(IC_SIZES, 5, seed=15)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        ps = [torch.tensor(a, dtype=dtype).requires_grad_() for a in p0]
        opt = torch.optim.AdamW(ps, lr=IC_LR, weight_decay=IC_WD, foreach=False)
        for gs in grads:
            for q, g in zip(ps, gs):
                q.grad = torch.tensor(g, dtype=dtype)
            opt.step()
        runs[dtype] = tuple(np.concatenate([t.detach().numpy() for t in ts])
                            for ts in (ps, [opt.state[q]["exp_avg"] for q in ps], [opt.state[q]["exp_avg_sq"] for q in ps]))
    flat = np.stack([np.concatenate(gs) for gs in grads])
    return p0, grads, runs[torch.float64], flat, fx.adamw_levels(runs[torch.float32], runs[torch.float64], flat, IC_LR)


def _steps(opt, params, grads):
    for gs in grads:
        for q, g in zip(params, gs):
            q.grad = torch.from_numpy(g).cuda()
        opt.step()


def _flat_state(opt, params):
    return tuple(np.concatenate([t.detach().cpu().numpy() for t in ts])
                 for ts in (params, [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params]))


@pytest.mark.parametrize("first", ["hip", "torch"])
def test_state_dicts_move_between_this_class_and_torch(hip, interchange_case, first):
    p0, grads, exact, flat, yard = interchange_case
    classes = {"hip": training.AdamW, "torch": torch.optim.AdamW}
    other = "torch" if first == "hip" else "hip"
    a = [torch.from_numpy(x).cuda().requires_grad_() for x in p0]
    opt_a = classes[first](a, lr=IC_LR, weight_decay=IC_WD)
    _steps(opt_a, a, grads[:3])
    b = [q.detach().clone().requires_grad_() for q in a]
    opt_b = classes[other](b, lr=IC_LR, weight_decay=IC_WD)
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))      # as through a checkpoint file: load_state_dict keeps the tensors it is given
    assert type(opt_b) is classes[other] and [float(opt_b.state[q]["step"]) for q in b] == [3.0] * len(b)
    _steps(opt_a, a, grads[3:])
    _steps(opt_b, b, grads[3:])
    for name, opt, params in ((first, opt_a, a), (other, opt_b, b)):
        assert [float(opt.state[q]["step"]) for q in params] == [5.0] * len(params)
        st = opt.state[params[0]]["step"]
        assert st.dtype == torch.float32 and st.device.type == "cpu"
        got = fx.adamw_levels(_flat_state(opt, params), exact, flat, IC_LR)
        print(f"{first} first, {name} side: levels {got}, torch float32 CPU levels {yard}")
        for k in ("p", "m", "v"):
            assert got[k] <= 3.0 * yard[k], (name, k, got[k], yard[k])


# ---- end to end
def test_two_training_rounds_of_the_detector(hip):
    """DBNet('resnet18', compute_threshold=True, trainable='head+fpn+layer4') at batch 2 on 640 x 640 frames (the one size this mode's frozen
    trunk engine takes), two training_step / backward / step rounds with optimizer='hip' against a deep copy driven by the default
    optimiser.  The two sides' gradients part in the last bits after the first update, so the comparison that carries a bound is a replay:
    torch.optim.AdamW in float64 and in float32 on the gradients the HIP side saw; the HIP result's levels may be at most 3x those of the
    float32 replay.  Against the copy: every trained tensor moves on both sides, frozen tensors keep their bits."""
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    lr, wd = 1e-4, 1e-5
    net = nets.DBNet("resnet18", compute_threshold=True, trainable="head+fpn+layer4")
    net.load_state_dict(stress_detector_state_dict("resnet18", 17))
    net.cuda().train()
    twin = copy.deepcopy(net)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = {"probability_map": (torch.rand((2, 1, 640, 640), generator=gen) < 0.2).float().cuda(),
               "threshold_map": (0.3 + 0.4 * torch.rand((2, 1, 640, 640), generator=gen)).cuda()}
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    seen, opts = [], {}
    for side, model, kw in (("hip", net, {"optimizer": "hip"}), ("torch", twin, {})):
        mod = training.TextDetectionLightningModule(model, learning_rate=lr, weight_decay=wd, **kw)
        opt = opts[side] = mod.configure_optimizers()["optimizer"]
        for rnd in range(2):
            loss = mod.training_step((x, targets), rnd)
            opt.zero_grad()
            loss.backward()
            if side == "hip":
                seen.append({k: p.grad.detach().cpu().numpy().ravel().copy() for k, p in model.named_parameters() if p.grad is not None})
            opt.step()
    assert type(opts["hip"]) is training.AdamW and type(opts["torch"]) is torch.optim.AdamW
    trained = sorted(seen[0])
    assert trained == sorted(seen[1]) and any(k.startswith("backbone.7.") for k in trained) and any(k.startswith("head.") for k in trained)
    after, after_twin = net.state_dict(), twin.state_dict()
    for k in trained:
        assert not torch.equal(before[k], after[k]) and not torch.equal(before[k], after_twin[k]), f"{k} did not move"
    frozen = [k for k, p in net.named_parameters() if k not in trained]
    assert any(k.startswith("backbone.4.") for k in frozen)
    for k in frozen:
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], after_twin[k]), f"{k} changed"
    # the replay of the HIP side's gradients through torch.optim.AdamW on the CPU
    grads = np.stack([np.concatenate([g[k] for k in trained]) for g in seen])
    runs = {}
    for dtype in (torch.float64, torch.float32):
        ps = [before[k].detach().cpu().to(dtype).reshape(-1).requires_grad_() for k in trained]
        opt = torch.optim.AdamW(ps, lr=lr, weight_decay=wd)
        for g in seen:
            for q, k in zip(ps, trained):
                q.grad = torch.from_numpy(g[k]).to(dtype)
            opt.step()
        runs[dtype] = tuple(np.concatenate([t.detach().numpy() for t in ts])
                            for ts in (ps, [opt.state[q]["exp_avg"] for q in ps], [opt.state[q]["exp_avg_sq"] for q in ps]))
    named = dict(net.named_parameters())
    hip_opt = opts["hip"]
    got = tuple(np.concatenate([t.detach().cpu().numpy().ravel() for t in ts])
                for ts in ([named[k] for k in trained], [hip_opt.state[named[k]]["exp_avg"] for k in trained],
                           [hip_opt.state[named[k]]["exp_avg_sq"] for k in trained]))
    lv, yard = fx.adamw_levels(got, runs[torch.float64], grads, lr), fx.adamw_levels(runs[torch.float32], runs[torch.float64], grads, lr)
    print(f"end to end, {grads.shape[1]} trained elements: HIP levels {lv}, torch float32 replay levels {yard}")
    for k in ("p", "m", "v"):
        assert lv[k] <= 3.0 * yard[k], (k, lv[k], yard[k])
    assert all(float(hip_opt.state[named[k]]["step"]) == 2.0 for k in trained)
    torch.cuda.synchronize()
    assert C.CDLL(_native.LIB_PATH).hipPeekAtLastError() == 0      # nothing pending in the process
