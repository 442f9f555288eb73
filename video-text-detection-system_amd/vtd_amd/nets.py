"""Parameter containers for DBNet and CRNN with the reference's state-dict key names.

The reference checkpoints are ``{'model_state_dict': sd}`` with keys laid out by
``nn.Sequential(*resnet.children()[:-2])`` / ``FeaturePyramidNetwork`` / ``DBHead``
(app/ml/models/text_detector.py:12-86) and ``CRNN`` (app/ml/models/text_recognizer.py:12-37);
SURVEY.md Appendix C lists them.  These modules reproduce exactly those keys and
shapes so ``load_state_dict(strict=True)`` accepts a reference checkpoint, but they
hold *parameters only*: ``forward`` hands the work to the HIP engine
(``vtd_amd.engine``), never to torch ops.

Repairs relative to the as-shipped reference: the
``'resnet18'`` channel plan exists (A2) and nothing is fetched from the network (A3).
"""
from collections import OrderedDict

import os
import threading

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable


def _conv_bn(cin, cout, k, stride, pad):
    return nn.Conv2d(cin, cout, k, stride, pad, bias=False), nn.BatchNorm2d(cout)


class _Residual(nn.Module):
    """Shared shell of the two ResNet v1.5 block kinds (parameters only)."""

    expansion = 1

    def forward(self, x):  # pragma: no cover - compute lives in the HIP engine
        raise RuntimeError("ResNet blocks are parameter containers; run DBNet.forward")


class BasicBlock(_Residual):
    expansion = 1

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv_bn(cin, width, 3, stride, 1)
        self.conv2, self.bn2 = _conv_bn(width, width, 3, 1, 1)
        self.stride = stride
        if stride != 1 or cin != width:
            self.downsample = nn.Sequential(*_conv_bn(cin, width, 1, stride, 0))


class Bottleneck(_Residual):
    expansion = 4

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv_bn(cin, width, 1, 1, 0)
        self.conv2, self.bn2 = _conv_bn(width, width, 3, stride, 1)  # v1.5: stride on the 3x3
        self.conv3, self.bn3 = _conv_bn(width, width * 4, 1, 1, 0)
        self.stride = stride
        if stride != 1 or cin != width * 4:
            self.downsample = nn.Sequential(*_conv_bn(cin, width * 4, 1, stride, 0))


_PLANS = {
    # name: (block class, blocks per stage, C5 channels)
    "resnet18": (BasicBlock, (2, 2, 2, 2), 512),
    "resnet50": (Bottleneck, (3, 4, 6, 3), 2048),
}


def make_trunk(name):
    """ResNet children()[:-2] as an 8-slot Sequential: 0 conv7x7/s2, 1 BN, 2 ReLU,
    3 maxpool, 4..7 the four stages (text_detector.py:17-19)."""
    block, counts, _ = _PLANS[name]
    slots = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
             nn.MaxPool2d(3, 2, 1)]
    cin = 64
    for stage, (n, width) in enumerate(zip(counts, (64, 128, 256, 512))):
        blocks = []
        for b in range(n):
            stride = 2 if (b == 0 and stage > 0) else 1
            blocks.append(block(cin, width, stride))
            cin = width * block.expansion
        slots.append(nn.Sequential(*blocks))
    return nn.Sequential(*slots)


def trunk_out_channels(name):
    return _PLANS[name][2]


class FeaturePyramidNetwork(nn.Module):
    """Same parameters as text_detector.py:31-41; the wiring (B.3 of SURVEY.md) is in the engine."""

    def __init__(self, in_channels):
        super().__init__()
        self.inner_blocks = nn.ModuleList(nn.Conv2d(in_channels >> i, 256, 1) for i in range(4))
        self.layer_blocks = nn.ModuleList(nn.Conv2d(256, 256, 3, padding=1) for _ in range(4))


def _db_branch(c):
    q = c // 4
    return nn.Sequential(
        nn.Conv2d(c, q, 3, padding=1), nn.BatchNorm2d(q), nn.ReLU(inplace=True),
        nn.ConvTranspose2d(q, q, 2, stride=2), nn.BatchNorm2d(q), nn.ReLU(inplace=True),
        nn.ConvTranspose2d(q, 1, 2, stride=2), nn.Sigmoid())


# per-branch tensors of the HIP training kernels (include/vtd.h vtd_dbhead_branch): (field, Sequential index, attribute)
_HEAD_FIELDS = (("conv_w", 0, "weight"), ("conv_b", 0, "bias"), ("bn1_w", 1, "weight"), ("bn1_b", 1, "bias"),
                ("bn1_mean", 1, "running_mean"), ("bn1_var", 1, "running_var"), ("ct1_w", 3, "weight"), ("ct1_b", 3, "bias"),
                ("bn2_w", 4, "weight"), ("bn2_b", 4, "bias"), ("bn2_mean", 4, "running_mean"), ("bn2_var", 4, "running_var"),
                ("ct2_w", 6, "weight"), ("ct2_b", 6, "bias"))
_HEAD_LEARNABLE = tuple(f for f in _HEAD_FIELDS if not f[2].startswith("running"))   # 10 per branch
_HEAD_BUFFERS = tuple(f for f in _HEAD_FIELDS if f[2].startswith("running"))


def _head_struct(tensors):
    """vtd_dbhead_params over a {(branch, field): tensor} mapping (missing fields stay NULL)."""
    import ctypes as C
    from . import _native
    st = _native.DbHeadParams()
    for (b, field), t in tensors.items():
        setattr(st.branch[b], field, C.c_void_p(t.data_ptr()))
    return st


class _DBHeadTrainFn(torch.autograd.Function):
    """DBHead.forward on the HIP training kernels (csrc/dbhead_train.hip), differentiable w.r.t. the 20 learnable head tensors.  Inputs:
    padded features (include/vtd.h), `src`, (H, W), BatchNorm mode / momentum / eps, the four running-stat buffers per branch (updated in
    place in training mode), then the learnable tensors branch-major in _HEAD_LEARNABLE order.  `src` is None, or the [n,256,H,W] tensor the
    padded features were packed from: when it requires grad the backward also forms the gradient of the features (dgrad into P2,
    vtd_dbhead_train_backward_input) and hands it to `src` in NCHW."""

    @staticmethod
    def forward(ctx, feats, src, hw, training, momentum, eps, buffers, *params):
        import ctypes as C
        from . import _native
        lib = _native.require()
        n, (H, W) = feats.shape[0], hw
        tensors = {}
        for b in range(2):
            for i, (field, _, _) in enumerate(_HEAD_LEARNABLE):
                tensors[(b, field)] = params[b * len(_HEAD_LEARNABLE) + i]
            for i, (field, _, _) in enumerate(_HEAD_BUFFERS):
                tensors[(b, field)] = buffers[b * len(_HEAD_BUFFERS) + i]
        st = _head_struct(tensors)
        dev = feats.device
        ws = torch.empty(int(lib.vtd_dbhead_train_workspace_bytes(n, H, W, 0)), dtype=torch.uint8, device=dev)
        prob = torch.empty((n, 1, 4 * H, 4 * W), dtype=torch.float32, device=dev)
        thresh = torch.empty_like(prob)
        stats = torch.empty((4, 2, 64), dtype=torch.float32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        _native.check(lib.vtd_dbhead_train_forward(ptr(feats), n, H, W, C.byref(st), 1 if training else 0, float(momentum), float(eps), ptr(ws),
                                                   ptr(prob), ptr(thresh), ptr(stats), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                      "vtd_dbhead_train_forward")
        ctx.save_for_backward(feats, prob, thresh, *params)
        ctx.ws, ctx.hw, ctx.training = ws, (H, W), bool(training)
        ctx.src_dtype = None if src is None else src.dtype
        ctx.mark_non_differentiable(stats)
        return prob, thresh, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_prob, grad_thresh, _grad_stats):
        import ctypes as C
        from . import _native
        lib = _native.require()
        feats, prob, thresh, *params = ctx.saved_tensors
        n, (H, W) = feats.shape[0], ctx.hw
        grads = [torch.empty_like(p) for p in params]
        tensors, gtensors = {}, {}
        for b in range(2):
            for i, (field, _, _) in enumerate(_HEAD_LEARNABLE):
                tensors[(b, field)] = params[b * len(_HEAD_LEARNABLE) + i]
                gtensors[(b, field)] = grads[b * len(_HEAD_LEARNABLE) + i]
        st, gst = _head_struct(tensors), _head_struct(gtensors)
        want_input = ctx.src_dtype is not None and ctx.needs_input_grad[1]
        scratch = torch.empty(int(lib.vtd_dbhead_train_workspace_bytes(n, H, W, 2 if want_input else 1)), dtype=torch.uint8, device=feats.device)
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (grad_prob, grad_thresh)]
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _native.check(lib.vtd_dbhead_train_backward(ptr(feats), n, H, W, C.byref(st), 1 if ctx.training else 0, ptr(ctx.ws), ptr(prob),
                                                    ptr(thresh), ptr(g[0]), ptr(g[1]), C.byref(gst), ptr(scratch),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_dbhead_train_backward")
        grad_src = None
        if want_input:
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            dfeats = torch.empty((n, H, W, 256), dtype=torch.float32, device=feats.device)   # NHWC, scaled by dscale[0]
            dscale = torch.empty(2, dtype=torch.float32, device=feats.device)
            _native.check(lib.vtd_dbhead_train_backward_input(n, H, W, C.byref(st), ptr(scratch), ptr(dfeats), ptr(dscale), stream),
                          "vtd_dbhead_train_backward_input")
            grad_src = torch.empty((n, 256, H, W), dtype=torch.float32, device=feats.device)
            _native.check(lib.vtd_dbhead_unpack_input_grad(ptr(dfeats), ptr(dscale), n, H, W, ptr(grad_src), stream), "vtd_dbhead_unpack_input_grad")
            grad_src = grad_src.to(ctx.src_dtype)
        return (None, grad_src, None, None, None, None, None, *grads)


def pack_features(features):
    """[n,256,H,W] float32 / float16 CUDA tensor -> padded features (ring-padded NHWC fp16 [n,H+2,W+2,256]) on the device."""
    import ctypes as C
    from . import _native
    lib = _native.require()
    x = features.detach()
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = x.contiguous()
    n, _, H, W = x.shape
    out = torch.empty((n, H + 2, W + 2, 256), dtype=torch.float16, device=x.device)
    _native.check(lib.vtd_dbhead_pack_features(C.c_void_p(x.data_ptr()), 0 if x.dtype == torch.float32 else 1, n, H, W,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "vtd_dbhead_pack_features")
    return out


class DBHead(nn.Module):
    """DBHead (text_detector.py:58-86).  ``head(features)`` on a CUDA ``[n,256,H,W]`` tensor returns ``{'probability', 'threshold'}``
    (``[n,1,4H,4W]`` fp32) from the HIP training kernels, with torch's BatchNorm semantics in ``train()`` (batch statistics, running
    statistics updated, ``num_batches_tracked`` + 1) and ``eval()``, differentiable w.r.t. the head's parameters.  A ``features`` tensor
    that requires grad is refused unless the call says ``input_grad=True``: then the backward also forms the gradient of the features
    (dgrad into P2, one more implicit GEMM) and ``features`` receives it in its own layout and dtype.  The head's parameter gradients are
    the same bits either way."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.probability_head = _db_branch(in_channels)
        self.threshold_head = _db_branch(in_channels)

    def _branches(self):
        return (self.probability_head, self.threshold_head)

    def forward(self, features, input_grad=False):
        if not torch.is_tensor(features) or features.dim() != 4 or features.shape[1] != self.in_channels:
            raise ValueError(f"DBHead input must be a [n,{self.in_channels},H,W] tensor")
        if features.requires_grad and not input_grad:
            raise RuntimeError("DBHead: the features require grad, but backward into the features (dgrad into P2) is only formed on "
                               "request; pass input_grad=True, or features.detach()")
        if not features.is_cuda:
            raise ValueError("DBHead runs on the HIP kernels: features must be a CUDA (HIP) tensor")
        src = features if input_grad and features.requires_grad and torch.is_grad_enabled() else None
        return self._forward_padded(pack_features(features), features.shape[2], features.shape[3], src)

    def forward_padded(self, feats, H, W):
        """The head on padded features (ring-padded NHWC fp16 [n,H+2,W+2,256], e.g. DetectorEngine.forward_features).  No gradient is
        formed for padded features (fp16 storage would flush it): the gradient of the features goes through ``forward(features,
        input_grad=True)``."""
        return self._forward_padded(feats, H, W, None)

    def _forward_padded(self, feats, H, W, src):
        if self.in_channels != 256:
            raise ValueError("the HIP DB-head kernels are specialised for 256 input channels")
        H, W = int(H), int(W)
        # the kernels trust the buffer's extent: a mismatch here would be a device-side out-of-bounds read
        if (not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float16 or not feats.is_contiguous() or feats.dim() != 4
                or H < 1 or W < 1 or feats.shape[0] < 1 or tuple(feats.shape[1:]) != (H + 2, W + 2, 256)):
            raise ValueError(f"padded features must be a contiguous float16 CUDA tensor [n,{H + 2},{W + 2},256] (H={H}, W={W}), got "
                             f"{tuple(feats.shape) if torch.is_tensor(feats) else type(feats).__name__}")
        bns = [seq[i] for seq in self._branches() for i in (1, 4)]
        if any(bn.momentum is None or bn.momentum != bns[0].momentum or bn.eps != bns[0].eps or not bn.track_running_stats for bn in bns):
            raise ValueError("the HIP DB-head kernels need one fixed momentum and eps on all four BatchNorms, with running stats tracked")
        params, buffers = [], []
        for seq in self._branches():
            params += [getattr(seq[i], a) for _, i, a in _HEAD_LEARNABLE]
            buffers += [getattr(seq[i], a) for _, i, a in _HEAD_BUFFERS]
        for t in params + buffers:
            if not t.is_cuda or t.device != feats.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("DBHead parameters and buffers must be contiguous float32 CUDA tensors on the features' device "
                                 "(call .cuda() on the model)")
        prob, thresh, _ = _DBHeadTrainFn.apply(feats, src, (int(H), int(W)), self.training, bns[0].momentum, bns[0].eps, tuple(buffers), *params)
        if self.training:
            with torch.no_grad():
                for bn in bns:
                    bn.num_batches_tracked.add_(1)
        return {"probability": prob, "threshold": thresh}


class _EngineOwner:
    """Engine bookkeeping shared by DBNet and CRNN.  The lock and the native handle are process-local: they are left out of
    pickles and deep copies (``copy.deepcopy(model)``, ``torch.save(model)``, multiprocessing spawn) and rebuilt on demand, so a
    copy packs its own engine from its own parameters at first use."""

    def _init_engine_state(self):
        self._engine = None
        self._engine_version = -1
        self._version = 0
        self._engine_lock = threading.Lock()

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None
        state["_engine_version"] = -1
        state.pop("_engine_lock", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._engine = None
        self._engine_version = -1
        self._engine_lock = threading.Lock()

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        new._engine_lock = threading.Lock()
        return new

    # any in-place parameter update through the public API invalidates the packed copy
    def load_state_dict(self, state_dict, strict=True, **kw):
        try:
            return super().load_state_dict(state_dict, strict=strict, **kw)
        finally:   # torch copies the matching tensors before it raises on a mismatch: the packed copy is stale either way
            self._version += 1

    def mark_dirty(self):
        self._version += 1


class DBNet(_EngineOwner, nn.Module):
    """DBNet detector network (text_detector.py:12-29), compute on the HIP engine.

    ``forward(x)`` accepts what the reference's ``TextDetector`` feeds it -- a
    normalised float NCHW tensor ``[B,3,640,640]`` -- or a ``DeviceFrames`` batch
    produced by the fused preprocess kernel, and returns
    ``{'probability': [B,1,640,640] f32 cuda tensor, 'threshold': same or None}``.
    """

    def __init__(self, backbone="resnet50", pretrained=False, compute_threshold=False, trainable=None):
        super().__init__()
        if backbone not in _PLANS:
            raise ValueError(f"unknown backbone {backbone!r}; expected one of {sorted(_PLANS)}")
        self.backbone_name = backbone
        self.backbone = make_trunk(backbone)
        self.fpn = FeaturePyramidNetwork(trunk_out_channels(backbone))
        self.head = DBHead(256)
        # the reference computes the threshold map and never reads it at inference
        # (text_detector.py:128); off by default, same kernels when switched on
        self.compute_threshold = compute_threshold
        self._init_engine_state()
        self.trainable = None
        self.set_trainable(trainable)

    def set_trainable(self, trainable):
        """None (default): forward-only on the fused inference engine, as always.  "head": fine-tune the DB head over a frozen trunk and
        FPN -- their parameters stop requiring grad, and a forward in train mode runs trunk + FPN on a separate features engine (built
        with fuse_fpn_head=0, rebuilt only when trunk / FPN weights change) and the head on the HIP training kernels, differentiable
        w.r.t. the head's parameters.  eval() forwards keep the fused inference engine, rebuilt after head updates."""
        if trainable not in (None, "head"):
            raise ValueError(f"trainable must be None or 'head', got {trainable!r}")
        self.trainable = trainable
        if trainable == "head":
            for p in list(self.backbone.parameters()) + list(self.fpn.parameters()):
                p.requires_grad_(False)
        self._head_versions = None
        return self

    def _head_tensor_versions(self):
        return tuple(t._version for t in list(self.head.parameters()) + list(self.head.buffers()))

    def features_engine(self):
        """The trunk + FPN engine of the trainable path (options fuse_fpn_head=0, see engine.DetectorEngine.forward_features)."""
        from . import engine as _e
        with self._engine_lock:
            # keyed on the trunk / FPN tensors' versions only (load_state_dict bumps them): head updates never rebuild it
            version = tuple(t._version for t in list(self.backbone.state_dict().values()) + list(self.fpn.state_dict().values()))
            fe = self.__dict__.get("_features_engine")
            if fe is None or self.__dict__.get("_features_version") != version:
                fe = _e.DetectorEngine(self.backbone_name, self.state_dict(), getattr(self, "_max_batch", None), options={"fuse_fpn_head": 0})
                self._features_engine, self._features_version = fe, version
            return fe

    def __getstate__(self):
        state = super().__getstate__()
        state["_features_engine"] = None
        return state

    def engine(self):
        """The native engine for the current parameters, built once under a lock (detect() is entered from four pool threads,
        pipeliine.py:32,96-101: without it a first mixed-size batch would build four engines).  A replaced engine is only
        dereferenced, never closed here: a thread still inside it keeps it alive and its handle is destroyed with the last
        reference."""
        from . import engine as _e
        with self._engine_lock:
            if self._engine is None or self._engine_version != self._version:
                version = self._version
                # VTD_DETECTOR_OPTIONS="fuse_fpn_head=0,fuse_stem_pool=0": build options for A/B measurements (include/vtd.h)
                opts = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("VTD_DETECTOR_OPTIONS", "").split(",") if kv)}
                self._engine = _e.DetectorEngine(self.backbone_name, self.state_dict(), getattr(self, "_max_batch", None),
                                                 options=opts or None)
                self._engine_version = version
            return self._engine

    def forward(self, x):
        if self.trainable == "head":
            if self.training:
                return self._forward_train_head(x)
            # the inference engine packs the head on the host: rebuild it after an optimizer step (parameter versions) or a
            # train-mode forward (running statistics, mark_dirty)
            versions = self._head_tensor_versions()
            if versions != self._head_versions:
                self._head_versions = versions
                self.mark_dirty()
        return self.engine().forward(x, want_threshold=self.compute_threshold)

    def _forward_train_head(self, x):
        frozen = [n for n, p in list(self.backbone.named_parameters(prefix="backbone")) + list(self.fpn.named_parameters(prefix="fpn"))
                  if p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable='head'): {frozen[0]} requires grad, but backward through the trunk / FPN is not "
                               "implemented; only the DB head trains (set requires_grad_(False) on backbone and fpn)")
        if not next(self.head.parameters()).is_cuda:
            self.head.cuda()   # the head's own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        feats = self.features_engine().forward_features(x)   # a new tensor per call: autograd may keep it
        out = self.head.forward_padded(feats, 160, 160)
        self.mark_dirty()   # the kernels updated the running statistics in place
        return out


class CRNN(_EngineOwner, nn.Module):
    """CRNN recogniser parameters (text_recognizer.py:12-37): 7 conv(+BN+ReLU) with the four
    pools, 2-layer bidirectional LSTM(512->256), Linear(512->vocab).  ``forward`` takes
    ``[B,3,32,128]`` float (BGR/255, text_recognizer.py:118-119) and returns ``[B,31,V]``
    logits as an f32 cuda tensor."""

    def __init__(self, vocab_size, hidden_size=256, num_layers=2):
        super().__init__()
        if hidden_size != 256 or num_layers != 2:
            raise ValueError("the HIP recogniser is specialised for hidden_size=256, num_layers=2")
        plan = [(3, 64, 3, 1, "p22"), (64, 128, 3, 1, "p22"), (128, 256, 3, 1, None),
                (256, 256, 3, 1, "p21"), (256, 512, 3, 1, None), (512, 512, 3, 1, "p21"),
                (512, 512, 2, 0, None)]
        mods = []
        for cin, cout, k, pad, pool in plan:
            mods += [nn.Conv2d(cin, cout, k, 1, pad), nn.BatchNorm2d(cout), nn.ReLU(True)]
            if pool == "p22":
                mods.append(nn.MaxPool2d(2, 2))
            elif pool == "p21":
                mods.append(nn.MaxPool2d((2, 1), (2, 1)))
        self.cnn = nn.Sequential(*mods)
        self.rnn = nn.LSTM(512, hidden_size, num_layers, batch_first=True, bidirectional=True)
        self.classifier = nn.Linear(hidden_size * 2, vocab_size)
        self.vocab_size = vocab_size
        self._init_engine_state()

    def engine(self):
        from . import engine as _e
        with self._engine_lock:   # see DBNet.engine
            if self._engine is None or self._engine_version != self._version:
                version = self._version
                self._engine = _e.RecognizerEngine(self.vocab_size, self.state_dict(), getattr(self, "_max_crops", None))
                self._engine_version = version
            return self._engine

    def forward(self, x):
        return self.engine().forward_logits(x)


def seeded_state_dict(module_factory, seed):
    """Deterministic default-init weights (torch's own init under a fixed seed) plus
    non-trivial BatchNorm statistics, so BN folding is actually exercised."""
    gen_state = torch.random.get_rng_state()
    try:
        torch.manual_seed(seed)
        m = module_factory()
        g = torch.Generator().manual_seed(seed + 7919)
        sd = OrderedDict()
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v = torch.randn(v.shape, generator=g) * 0.05
            elif k.endswith("running_var"):
                v = 1.0 + 0.2 * torch.rand(v.shape, generator=g)
            elif k.endswith("num_batches_tracked"):
                v = v.clone()
            elif v.dim() == 1 and _is_bn_gamma(k, m):
                v = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
            sd[k] = v.clone()
        return sd
    finally:
        torch.random.set_rng_state(gen_state)


def _is_bn_gamma(key, module):
    if not key.endswith(".weight"):
        return False
    owner = module
    for part in key.split(".")[:-1]:
        owner = getattr(owner, part) if not part.isdigit() else owner[int(part)]
    return isinstance(owner, nn.BatchNorm2d)
