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
from collections import OrderedDict, namedtuple

import os
import threading

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable


def _conv_bn(cin, cout, k, stride, pad):
    return nn.Conv2d(cin, cout, k, stride, pad, bias=False), nn.BatchNorm2d(cout)


def _native_workspace(query, args, device):
    """The preamble of the raw wrappers of the training kernels: (ctypes, _native, the loaded library, a byte buffer on `device` of the size
    the library's `query`(*args) asks for).  A negative size is the library's refusal of the arguments and raises its text."""
    import ctypes
    from . import _native
    lib = _native.require()
    nbytes = int(getattr(lib, query)(*args))
    _native.check(min(nbytes, 0), query)
    return ctypes, _native, lib, torch.empty(nbytes, dtype=torch.uint8, device=device)


class _Residual(nn.Module):
    """Shared shell of the two ResNet v1.5 block kinds (parameters only)."""

    expansion = 1

    def forward(self, x):  # pragma: no cover - compute lives in the HIP engine
        raise RuntimeError("ResNet blocks are parameter containers; run DBNet.forward")


class BasicBlock(_Residual):
    """ResNet BasicBlock.  ``block(x)`` on a CUDA NCHW tensor (fp32 or fp16) runs the block on the HIP training kernels
    (csrc/resblock_train.hip) with frozen-statistics BatchNorm -- the running statistics normalise and are never written, whatever
    ``training`` says -- and returns ``[n,width,h,w]`` fp32, differentiable w.r.t. the block's learnable tensors (convolution weights,
    BatchNorm gamma and beta) and, for the stride-1 block, w.r.t. ``x``.  Built geometries: ResNet-18's layer4 (256 -> 512 stride 2 with
    downsample and even extents, 512 -> 512 stride 1)."""
    expansion = 1

    def __init__(self, cin, width, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv_bn(cin, width, 3, stride, 1)
        self.conv2, self.bn2 = _conv_bn(width, width, 3, 1, 1)
        self.stride = stride
        if stride != 1 or cin != width:
            self.downsample = nn.Sequential(*_conv_bn(cin, width, 1, stride, 0))

    def _train_operands(self, device, general=False, narrow=False):
        """((cin, width, stride), eps, the learnable tensors, the running statistics) as the kernels take them, validated.  `general`: the
        six geometries of the vtd_resblock_train_* entries (layer2's, layer3's and layer4's) instead of layer4's two.  `narrow`: layer1's
        64 -> 64 stride-1 block (the vtd_block64_train_* entries) is admitted too; every other geometry is judged as without it."""
        cin, width = self.conv1.in_channels, self.conv1.out_channels
        ds = hasattr(self, "downsample")
        if narrow and (cin, width, self.stride, ds) == _BLOCK64_GEOMETRY:
            pass
        elif general and (cin, width, self.stride, ds) not in _BLOCK_GEOMETRIES:
            raise RuntimeError(f"BasicBlock({cin} -> {width}, stride {self.stride}): basic_block_train is built for ResNet-18's layer2, layer3 and layer4 "
                               "(64 -> 128, 128 -> 256 and 256 -> 512 stride 2 with downsample, 128 -> 128, 256 -> 256 and 512 -> 512 stride 1)")
        elif not general and (cin, width, self.stride, ds) not in ((256, 512, 2, True), (512, 512, 1, False)):
            raise RuntimeError(f"BasicBlock({cin} -> {width}, stride {self.stride}): the HIP training kernels are built for ResNet-18's layer4 only "
                               "(256 -> 512 stride 2 with downsample, 512 -> 512 stride 1)")
        pairs = [(self.conv1, self.bn1), (self.conv2, self.bn2)] + ([(self.downsample[0], self.downsample[1])] if ds else [])
        if any(bn.eps != self.bn1.eps or not bn.track_running_stats for _, bn in pairs):
            raise ValueError("the HIP BasicBlock kernels need one eps on all BatchNorms, with running stats tracked")
        learn, stats = [], []
        for conv, bn in pairs:
            learn += [conv.weight, bn.weight, bn.bias]
            stats += [bn.running_mean, bn.running_var]
        for t in learn + stats:
            if not t.is_cuda or t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("BasicBlock parameters and buffers must be contiguous float32 CUDA tensors on the input's device "
                                 "(call .cuda() on the model)")
        return (cin, width, self.stride), float(self.bn1.eps), learn, stats

    def forward(self, x):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.conv1.in_channels:
            raise ValueError(f"BasicBlock input must be a [n,{self.conv1.in_channels},H,W] tensor")
        if not x.is_cuda:
            raise ValueError("BasicBlock runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
        (cin, width, stride), eps, learn, stats = self._train_operands(x.device)
        n, _, hin, win = x.shape
        if n < 1 or hin < 1 or win < 1 or (stride == 2 and (hin % 2 or win % 2)):
            raise RuntimeError(f"BasicBlock(stride {stride}): the HIP training kernels need a non-empty input with even extents, got {tuple(x.shape)}")
        if stride != 1 and x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("BasicBlock(stride 2): the input requires grad, but the input gradient of the stride-2 block (a strided dgrad) is "
                               "not built; pass x.detach()")
        src = x if x.requires_grad and torch.is_grad_enabled() else None
        return _BlockTrainFn.apply(pack_tap(x), src, (int(n), int(hin), int(win), cin, width, stride), eps, tuple(stats), _BASICBLOCK, None, *learn)


_BLOCK_GEOMETRIES = ((64, 128, 2, True), (128, 128, 1, False), (128, 256, 2, True), (256, 256, 1, False), (256, 512, 2, True), (512, 512, 1, False))
_BLOCK64_GEOMETRY = (64, 64, 1, False)   # layer1's, behind entries of its own


# the geometries with train-mode (batch-statistics) BatchNorm built (csrc/resblock_bn_train.hip): ResNet-18's layer4
_BN_TRAIN_GEOMETRIES = ((256, 512, 2, True), (512, 512, 1, False))
_BN_TRAIN_BUILT = ("train-mode (batch-statistics) BatchNorm is built for the BasicBlocks of ResNet-18's layer4 only (256 -> 512 stride 2 with "
                   "downsample, 512 -> 512 stride 1); layer3, layer2, layer1, the stem and Bottleneck blocks keep frozen statistics")


# the same on the vtd_block_bn_train_* entries: layer3's two geometries too, and the input gradient of either stride
_BLOCK_BN_GEOMETRIES = ((128, 256, 2, True), (256, 256, 1, False)) + _BN_TRAIN_GEOMETRIES
_BLOCK_BN_BUILT = ("basic_block_bn_train (train-mode, batch-statistics BatchNorm) is built for the BasicBlocks of ResNet-18's layer3 and layer4 "
                   "(128 -> 256 and 256 -> 512 stride 2 with downsample, 256 -> 256 and 512 -> 512 stride 1); layer2, layer1, the stem and "
                   "Bottleneck blocks keep frozen statistics")
# the stages whose BatchNorms the trunk node can run with batch statistics (forward_padded's trunk_batch_stats, DBNet's trunk_bn), with the
# training mode each goes with
_TRUNK_BN_STAGES = {("layer4",): "head+fpn+layer4", ("layer3", "layer4"): "head+fpn+layer4+layer3"}
_TRUNK_BN_BUILT = ("train-mode (batch-statistics) trunk BatchNorm is built for ('layer4',) with trainable='head+fpn+layer4' and for "
                   "('layer3', 'layer4') with trainable='head+fpn+layer4+layer3', on resnet18; the tuple names exactly the residual stages that "
                   "train; layer2, layer1 and the stem keep frozen statistics under a tuple; with layer2 too the spellings are "
                   "forward_padded(..., trunk_batch_stats=('layer2', 'layer3', 'layer4')) and DBNet(trainable='head+fpn+layer4+layer3+layer2', "
                   "trunk_bn='trained'), with layer1 too forward_padded(..., trunk_batch_stats=('layer1', 'layer2', 'layer3', 'layer4')) and "
                   "DBNet(trainable='head+fpn+layer4+layer3+layer2+layer1', trunk_bn='trained')")
# the same on the vtd_trunk_bn_train_* entries, the family later stages join: layer2's two geometries and layer1's one too
_TRUNK_BLOCK_BN_GEOMETRIES = ((64, 64, 1, False), (64, 128, 2, True), (128, 128, 1, False)) + _BLOCK_BN_GEOMETRIES
_TRUNK_BLOCK_BN_BUILT = ("trunk_block_bn_train (train-mode, batch-statistics BatchNorm) is built for the BasicBlocks of ResNet-18's layer1, layer2, "
                         "layer3 and layer4 (64 -> 64 stride 1, 64 -> 128, 128 -> 256 and 256 -> 512 stride 2 with downsample, 128 -> 128, "
                         "256 -> 256 and 512 -> 512 stride 1); the stem and Bottleneck blocks keep frozen statistics")
# the stage tuples forward_padded's trunk_batch_stats takes; the last two are the layer2 -> layer3 -> layer4 -> FPN -> head node and the
# layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head node, which DBNet spells trunk_bn="trained"
_NODE_BN_STAGES = (("layer4",), ("layer3", "layer4"), ("layer2", "layer3", "layer4"), ("layer1", "layer2", "layer3", "layer4"))
# DBNet's trunk_bn="trained": every residual stage the mode trains runs its BatchNorms in train mode
_TRAINED_BN_MODES = ("head+fpn+layer4", "head+fpn+layer4+layer3", "head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3+layer2+layer1")
_TRAINED_BN_BUILT = ("trunk_bn='trained' (train-mode, batch-statistics BatchNorm in every residual stage the mode trains) is built for "
                     "trainable='head+fpn+layer4', 'head+fpn+layer4+layer3', 'head+fpn+layer4+layer3+layer2' and "
                     "'head+fpn+layer4+layer3+layer2+layer1' on resnet18; the stem keeps frozen statistics under 'trained': "
                     "DBNet(trainable='head+fpn+backbone', trunk_bn='backbone') is the spelling that trains the stem's statistics too")
# DBNet's trunk_bn="backbone": all twenty BatchNorms of the trunk, the stem's too (csrc/stem_train.hip: vtd_stem_bn_train_*), in train mode
_BACKBONE_BN_BUILT = ("trunk_bn='backbone' (train-mode, batch-statistics BatchNorm in the stem and in every residual stage) is built for "
                      "trainable='head+fpn+backbone' on resnet18")


def _block_bn_check(block, geometries=_BN_TRAIN_GEOMETRIES, built=_BN_TRAIN_BUILT):
    """The BatchNorms of a BasicBlock that vtd_resblock_bn_train_* (or, with the four `geometries`, vtd_block_bn_train_*) can run in train
    mode (bn1, bn2, the downsample's), validated."""
    cin, width, ds = block.conv1.in_channels, block.conv1.out_channels, hasattr(block, "downsample")
    if (cin, width, block.stride, ds) not in geometries:
        raise RuntimeError(f"BasicBlock({cin} -> {width}, stride {block.stride}): " + built)
    bns = [block.bn1, block.bn2] + ([block.downsample[1]] if ds else [])
    if any(bn.momentum is None or bn.momentum != bns[0].momentum for bn in bns):
        raise ValueError("the HIP batch-statistics BasicBlock kernels need one fixed momentum on all of the block's BatchNorms "
                         "(momentum=None, the cumulative average, is not built)")
    return bns


def basic_block_train(block, x, batch_stats=False):
    """With ``batch_stats=True`` (layer4's two geometries only, csrc/resblock_bn_train.hip) the block's BatchNorms behave as torch's
    modules do: in ``block.training`` mode the statistics of the batch normalise, the running statistics are updated in place and
    ``num_batches_tracked`` advances on each of the block's BatchNorms; in ``eval()`` mode the frozen path below runs, the same bits.  The
    stride-2 block forms no input gradient on this path: an input that requires grad is refused.

    One BasicBlock on the HIP training kernels (csrc/resblock_train.hip) as a differentiable function of a CUDA NCHW tensor (fp32 or
    fp16), for the seven blocks of ResNet-18's four stages: 64 -> 64 at stride 1 (layer1's, on the vtd_block64_train_* entries), and on the
    vtd_resblock_train_* entries 64 -> 128, 128 -> 256 and 256 -> 512 at stride 2 (with downsample, even extents), 128 -> 128, 256 -> 256
    and 512 -> 512 at stride 1.  Frozen-statistics BatchNorm, as ``block(x)``; returns ``[n,width,h,w]`` fp32, differentiable w.r.t. the
    block's learnable tensors and w.r.t. ``x`` for either stride (the stride-2 blocks through the strided dgrad).  For layer4's blocks the
    output and the parameter gradients are the bits of ``block(x)``."""
    if not isinstance(block, BasicBlock):
        raise RuntimeError("basic_block_train is built for ResNet-18's BasicBlocks; Bottleneck training is not built here "
                           "(ResNet-50's last stage goes to bottleneck_train)")
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != block.conv1.in_channels:
        raise ValueError(f"BasicBlock input must be a [n,{block.conv1.in_channels},H,W] tensor")
    bns = _block_bn_check(block) if batch_stats else None   # what is built, before anything about the device
    if not x.is_cuda:
        raise ValueError("BasicBlock runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
    if batch_stats:
        return _basic_block_bn_train(block, x, bns)
    (cin, width, stride), eps, learn, stats = block._train_operands(x.device, general=True, narrow=True)
    n, _, hin, win = x.shape
    if n < 1 or hin < 1 or win < 1 or (stride == 2 and (hin % 2 or win % 2)):
        raise RuntimeError(f"BasicBlock(stride {stride}): the HIP training kernels need a non-empty input with even extents, got {tuple(x.shape)}")
    src = x if x.requires_grad and torch.is_grad_enabled() else None
    geom = (int(n), int(hin), int(win), cin, width, stride)
    return _BlockTrainFn.apply(pack_tap(x), src, geom, eps, tuple(stats), _block_entry(geom), None, *learn)


def basic_block_bn_train(block, x):
    """One BasicBlock of ResNet-18's layer3 or layer4 (128 -> 256 and 256 -> 512 at stride 2 with downsample and even extents, 256 -> 256 and
    512 -> 512 at stride 1) on the vtd_block_bn_train_* entries (csrc/resblock_bn_train.hip) with torch's module semantics: in
    ``block.training`` mode the statistics of the batch normalise, the running statistics are updated in place and ``num_batches_tracked``
    advances on each of the block's BatchNorms; in ``eval()`` mode it gives the bits of ``basic_block_train(block, x)``.  Returns
    ``[n,width,h,w]`` fp32, differentiable w.r.t. the block's learnable tensors and w.r.t. ``x`` for either stride (the stride-2 blocks
    through the strided dgrad of dz1 plus the downsample's transpose of its own dz).  For layer4's blocks the output, the parameter
    gradients, the running update and the stride-1 input gradient are the bits of ``basic_block_train(block, x, batch_stats=True)``."""
    if not isinstance(block, BasicBlock):
        raise RuntimeError("basic_block_bn_train: Bottleneck training is not built; " + _BLOCK_BN_BUILT)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != block.conv1.in_channels:
        raise ValueError(f"BasicBlock input must be a [n,{block.conv1.in_channels},H,W] tensor")
    bns = _block_bn_check(block, _BLOCK_BN_GEOMETRIES, _BLOCK_BN_BUILT)   # what is built, before anything about the device
    if not x.is_cuda:
        raise ValueError("BasicBlock runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
    return _basic_block_bn_train(block, x, bns, general=True)


def trunk_block_bn_train(block, x):
    """``basic_block_bn_train`` on the vtd_trunk_bn_train_* entries, the family later stages join: layer2's two geometries too (64 -> 128 at
    stride 2 with downsample and even extents, 128 -> 128 at stride 1) and layer1's 64 -> 64 at stride 1, seven in all.  The same module
    semantics: ``block.training`` selects batch or frozen statistics, the block's BatchNorms need one fixed momentum, the running statistics are updated in place and
    ``num_batches_tracked`` advances in train mode, and the result is differentiable w.r.t. the block's learnable tensors and w.r.t. ``x``
    at either stride.  For the four geometries of layer3 and layer4 every output is the bits of ``basic_block_bn_train``; in ``eval()``
    mode it gives the bits of ``basic_block_train(block, x)`` and writes no buffer."""
    if not isinstance(block, BasicBlock):
        raise RuntimeError("trunk_block_bn_train: Bottleneck training is not built; " + _TRUNK_BLOCK_BN_BUILT)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != block.conv1.in_channels:
        raise ValueError(f"BasicBlock input must be a [n,{block.conv1.in_channels},H,W] tensor")
    bns = _block_bn_check(block, _TRUNK_BLOCK_BN_GEOMETRIES, _TRUNK_BLOCK_BN_BUILT)   # what is built, before anything about the device
    if not x.is_cuda:
        raise ValueError("BasicBlock runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
    return _basic_block_bn_train(block, x, bns, general=True, entry=_TRUNK_BN, narrow=True)


def _basic_block_bn_train(block, x, bns, general=False, entry=None, narrow=False):
    (cin, width, stride), eps, learn, stats = block._train_operands(x.device, general=general, narrow=narrow)
    n, _, hin, win = x.shape
    if n < 1 or hin < 1 or win < 1 or (stride == 2 and (hin % 2 or win % 2)):
        raise RuntimeError(f"BasicBlock(stride {stride}): the HIP training kernels need a non-empty input with even extents, got {tuple(x.shape)}")
    if block.training and n * (hin // stride) * (win // stride) < 2:
        raise ValueError(f"train-mode BatchNorm needs more than one value per channel, got an output of {n} x {hin // stride} x {win // stride}")
    if not general and stride != 1 and x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("BasicBlock(stride 2, batch_stats=True): the input requires grad, but the input gradient of the stride-2 block is not "
                           "built with batch-statistics BatchNorm; pass x.detach()")
    src = x if x.requires_grad and torch.is_grad_enabled() else None
    out = _BlockTrainFn.apply(pack_tap(x), src, (int(n), int(hin), int(win), cin, width, stride), eps, tuple(stats),
                              entry or (_BLOCK_BN if general else _RESBLOCK_BN), (bool(block.training), float(bns[0].momentum)), *learn)
    if block.training:
        with torch.no_grad():
            for bn in bns:
                bn.num_batches_tracked.add_(1)
    return out


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


# the Bottleneck geometries csrc/bottleneck_train.hip builds: ResNet-50's last stage (res5, torchvision's layer4), (cin, width, stride, downsample)
_BOTTLENECK_GEOMETRIES = ((1024, 512, 2, True), (2048, 512, 1, False))
_BOTTLENECK_BUILT = ("bottleneck_train is built for the Bottlenecks of ResNet-50's last stage, res5 (1024 -> 512 -> 2048 stride 2 with downsample and "
                     "even extents, 2048 -> 512 -> 2048 stride 1), with frozen-statistics BatchNorm")
_RES5_BUILT = ("res5 training is built for ResNet-50's last stage: three Bottlenecks of width 512 (1024 -> 2048 stride 2 with downsample, then "
               "2048 -> 2048 stride 1, twice) on a C4 tap of 1024 channels and even extents, with one BatchNorm eps")


# ResNet-50's res4 (torchvision's layer3): the 256-wide Bottlenecks, behind the vtd_bottleneck256_train_* entries of the same file
_BOTTLENECK256_GEOMETRIES = ((512, 256, 2, True), (1024, 256, 1, False))
_BOTTLENECK256_BUILT = ("bottleneck256_train is built for the Bottlenecks of ResNet-50's res4 (512 -> 256 -> 1024 stride 2 with downsample and "
                        "even extents, 1024 -> 256 -> 1024 stride 1), with frozen-statistics BatchNorm")
_RES4_BUILT = ("res4 training is built for ResNet-50's res4: six Bottlenecks of width 256 (512 -> 1024 stride 2 with downsample, then "
               "1024 -> 1024 stride 1, five times) on a C3 tap of 512 channels and even extents, with one BatchNorm eps")


# ResNet-50's res3 (torchvision's layer2): the 128-wide Bottlenecks, behind the vtd_bottleneck128_train_* entries of the same file
_BOTTLENECK128_GEOMETRIES = ((256, 128, 2, True), (512, 128, 1, False))
_BOTTLENECK128_BUILT = ("bottleneck128_train is built for the Bottlenecks of ResNet-50's res3 (256 -> 128 -> 512 stride 2 with downsample and "
                        "even extents, 512 -> 128 -> 512 stride 1), with frozen-statistics BatchNorm")
_RES3_BUILT = ("res3 training is built for ResNet-50's res3: four Bottlenecks of width 128 (256 -> 512 stride 2 with downsample, then "
               "512 -> 512 stride 1, three times) on a C2 tap of 256 channels and even extents, with one BatchNorm eps")


# ResNet-50's res2 (torchvision's layer1): the 64-wide Bottlenecks, behind the vtd_bottleneck64_train_* entries of the same file.  Both
# geometries run at stride 1; the first block's downsample is a 1x1 convolution at stride 1 over the pooled stem output's 64 channels
_BOTTLENECK64_GEOMETRIES = ((64, 64, 1, True), (256, 64, 1, False))
_BOTTLENECK64_BUILT = ("bottleneck64_train is built for the Bottlenecks of ResNet-50's res2 (64 -> 64 -> 256 stride 1 with downsample, "
                       "256 -> 64 -> 256 stride 1), with frozen-statistics BatchNorm")
_RES2_BUILT = ("res2 training is built for ResNet-50's res2: three Bottlenecks of width 64 (64 -> 256 stride 1 with downsample, then "
               "256 -> 256 stride 1, twice) on a pooled tap of 64 channels, with one BatchNorm eps")


def _bottleneck_pairs(block):
    return ([(block.conv1, block.bn1), (block.conv2, block.bn2), (block.conv3, block.bn3)] +
            ([(block.downsample[0], block.downsample[1])] if hasattr(block, "downsample") else []))


def _bottleneck_check(block, geometries=_BOTTLENECK_GEOMETRIES, built=_BOTTLENECK_BUILT):
    """((cin, width, stride), eps) of a Bottleneck that csrc/bottleneck_train.hip runs under one entry family (`geometries`: res5's by default,
    res4's with _BOTTLENECK256_GEOMETRIES), judged without looking at any device."""
    if not isinstance(block, Bottleneck):
        raise RuntimeError(f"{type(block).__name__}: " + built + " (a BasicBlock goes to basic_block_train)")
    cin, width = block.conv1.in_channels, block.conv1.out_channels
    if (cin, width, block.stride, hasattr(block, "downsample")) not in geometries:
        raise RuntimeError(f"Bottleneck({cin} -> {width} -> {4 * width}, stride {block.stride}): " + built)
    if any(bn.eps != block.bn1.eps or not bn.track_running_stats for _, bn in _bottleneck_pairs(block)):
        raise ValueError("the HIP Bottleneck kernels need one eps on all BatchNorms, with running stats tracked")
    return (cin, width, block.stride), float(block.bn1.eps)


def _bottleneck_operands(block, device, geometries=_BOTTLENECK_GEOMETRIES, built=_BOTTLENECK_BUILT):
    """((cin, width, stride), eps, the 9 or 12 learnable tensors, the running statistics) as vtd_bottleneck_train_* (or, with res4's
    geometries, vtd_bottleneck256_train_*) take them, validated."""
    geom, eps = _bottleneck_check(block, geometries, built)
    learn, stats = [], []
    for conv, bn in _bottleneck_pairs(block):
        learn += [conv.weight, bn.weight, bn.bias]
        stats += [bn.running_mean, bn.running_var]
    for t in learn + stats:
        if not t.is_cuda or t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("Bottleneck parameters and buffers must be contiguous float32 CUDA tensors on the input's device "
                             "(call .cuda() on the model)")
    return geom, eps, learn, stats


def bottleneck_train(block, x):
    """One Bottleneck of ResNet-50's last stage on the HIP training kernels (csrc/bottleneck_train.hip) as a differentiable function of a CUDA
    NCHW tensor (fp32 or fp16): 1024 -> 512 -> 2048 at stride 2 (with downsample, even extents) or 2048 -> 512 -> 2048 at stride 1.
    Frozen-statistics BatchNorm -- the running statistics normalise and are never written, whatever ``training`` says.  Returns
    ``[n,2048,h,w]`` fp32, differentiable w.r.t. the block's 12 or 9 learnable tensors and w.r.t. ``x`` at either stride.  Everything else is
    refused before the device is looked at."""
    return _bottleneck_train(block, x, _BOTTLENECK_GEOMETRIES, _BOTTLENECK_BUILT, _BOTTLENECK)


def bottleneck256_train(block, x):
    """bottleneck_train's counterpart for ResNet-50's res4 (the vtd_bottleneck256_train_* entries): 512 -> 256 -> 1024 at stride 2 (with
    downsample, even extents) or 1024 -> 256 -> 1024 at stride 1.  Returns ``[n,1024,h,w]`` fp32, differentiable w.r.t. the block's 12 or 9
    learnable tensors and w.r.t. ``x`` at either stride; frozen statistics, never written; the same refusals before the device is looked at."""
    return _bottleneck_train(block, x, _BOTTLENECK256_GEOMETRIES, _BOTTLENECK256_BUILT, _BOTTLENECK256)


def bottleneck128_train(block, x):
    """bottleneck_train's counterpart for ResNet-50's res3 (the vtd_bottleneck128_train_* entries): 256 -> 128 -> 512 at stride 2 (with
    downsample, even extents) or 512 -> 128 -> 512 at stride 1.  Returns ``[n,512,h,w]`` fp32, differentiable w.r.t. the block's 12 or 9
    learnable tensors and w.r.t. ``x`` at either stride; frozen statistics, never written; the same refusals before the device is looked at."""
    return _bottleneck_train(block, x, _BOTTLENECK128_GEOMETRIES, _BOTTLENECK128_BUILT, _BOTTLENECK128)


def bottleneck64_train(block, x):
    """bottleneck_train's counterpart for ResNet-50's res2 (the vtd_bottleneck64_train_* entries): 64 -> 64 -> 256 (with a 1x1 downsample at
    stride 1) or 256 -> 64 -> 256, both at stride 1.  Returns ``[n,256,h,w]`` fp32, differentiable w.r.t. the block's 12 or 9 learnable
    tensors and w.r.t. ``x`` for either geometry; frozen statistics, never written; the same refusals before the device is looked at."""
    return _bottleneck_train(block, x, _BOTTLENECK64_GEOMETRIES, _BOTTLENECK64_BUILT, _BOTTLENECK64)


# the Bottleneck geometries with train-mode (batch-statistics) BatchNorm built (csrc/bottleneck_bn_train.hip): ResNet-50's res5 and res4
_BOTTLENECK_BN_GEOMETRIES = _BOTTLENECK_GEOMETRIES + _BOTTLENECK256_GEOMETRIES
_BOTTLENECK_BN_BUILT = ("bottleneck_bn_train (train-mode, batch-statistics BatchNorm) is built for the Bottlenecks of ResNet-50's res5 and res4 "
                        "(1024 -> 512 -> 2048 and 512 -> 256 -> 1024 stride 2 with downsample and even extents, 2048 -> 512 -> 2048 and "
                        "1024 -> 256 -> 1024 stride 1); res3, res2 and the stem keep frozen statistics")
_RES_BN_BUILT = ("batch-statistics BatchNorm in Bottleneck stages is built for ResNet-50's res5 and res4: forward_padded(..., res5=, "
                 "res_batch_stats=True) on the taps [C2, C3, C4] and forward_padded(..., res5=, res4=, res_batch_stats=True) on [C2, C3], and "
                 "DBNet('resnet50', trainable='head+fpn+res5' or 'head+fpn+res5+res4', trunk_bn='bottleneck'); res3, res2 and the stem keep "
                 "frozen statistics")
_BOTTLENECK_BN_MOMENTUM = ("the HIP batch-statistics Bottleneck kernels need one fixed momentum on all of the block's BatchNorms "
                           "(momentum=None, the cumulative average, is not built)")


def _bottleneck_bn_check(block):
    """((cin, width, stride), eps, the block's BatchNorms, their momentum) of a Bottleneck that vtd_bottleneck_bn_train_* can run in train
    mode, judged without looking at any device."""
    geom, eps = _bottleneck_check(block, _BOTTLENECK_BN_GEOMETRIES, _BOTTLENECK_BN_BUILT)
    bns = [bn for _, bn in _bottleneck_pairs(block)]
    if any(bn.momentum is None or bn.momentum != bns[0].momentum for bn in bns):
        raise ValueError(_BOTTLENECK_BN_MOMENTUM)
    return geom, eps, bns, float(bns[0].momentum)


def bottleneck_bn_train(block, x):
    """One Bottleneck of ResNet-50's res5 or res4 (1024 -> 512 -> 2048 and 512 -> 256 -> 1024 at stride 2 with downsample and even extents,
    2048 -> 512 -> 2048 and 1024 -> 256 -> 1024 at stride 1) on the vtd_bottleneck_bn_train_* entries (csrc/bottleneck_bn_train.hip) with
    torch's module semantics: in ``block.training`` mode the statistics of the batch normalise, the running statistics are updated in place
    and ``num_batches_tracked`` advances on each of the block's three or four BatchNorms; in ``eval()`` mode it gives the bits of
    ``bottleneck_train`` / ``bottleneck256_train`` and writes no buffer.  The block's BatchNorms need one eps and one fixed momentum.
    Returns ``[n,4 width,h,w]`` fp32, differentiable w.r.t. the block's 12 or 9 learnable tensors and w.r.t. ``x`` at either stride.
    Everything else is refused before the device is looked at."""
    geom, eps, bns, momentum = _bottleneck_bn_check(block)
    n, hin, win = _bottleneck_input(x, geom, batch=block.training)
    _, _, learn, stats = _bottleneck_operands(block, x.device, _BOTTLENECK_BN_GEOMETRIES, _BOTTLENECK_BN_BUILT)
    src = x if x.requires_grad and torch.is_grad_enabled() else None
    out = _BlockTrainFn.apply(pack_tap(x), src, (n, hin, win, *geom), eps, tuple(stats), _BOTTLENECK_BN, (bool(block.training), momentum), *learn)
    if block.training:
        with torch.no_grad():
            for bn in bns:
                bn.num_batches_tracked.add_(1)
    return out


def _bottleneck_input(x, geom, batch=False):
    """(n, H, W) of the input of a single Bottleneck of geometry (cin, width, stride), checked in the wrappers' order; `batch`: the block
    normalises with the statistics of the batch, which needs more than one value per channel."""
    cin, _, stride = geom
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != cin:
        raise ValueError(f"Bottleneck input must be a [n,{cin},H,W] tensor")
    n, _, hin, win = x.shape
    if n < 1 or hin < 1 or win < 1 or (stride == 2 and (hin % 2 or win % 2)):
        raise RuntimeError(f"Bottleneck(stride {stride}): the HIP training kernels need a non-empty input with even extents, got {tuple(x.shape)}")
    if batch and n * (hin // stride) * (win // stride) < 2:
        raise ValueError(f"train-mode BatchNorm needs more than one value per channel, got an output of {n} x {hin // stride} x {win // stride}")
    if not x.is_cuda:
        raise ValueError("Bottleneck runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
    return int(n), int(hin), int(win)


def _bottleneck_train(block, x, geometries, built, entry):
    geom, eps = _bottleneck_check(block, geometries, built)
    n, hin, win = _bottleneck_input(x, geom)
    _, _, learn, stats = _bottleneck_operands(block, x.device, geometries, built)
    src = x if x.requires_grad and torch.is_grad_enabled() else None
    return _BlockTrainFn.apply(pack_tap(x), src, (n, hin, win, *geom), eps, tuple(stats), entry, None, *learn)


def _res_operands(stage, layer, tap, device=None):
    """One stage of ResNet-50 (a row of _RES_STAGES) on a padded tap of its input: (the blocks, their geometries, eps, their learnable
    tensors, their running statistics).  Only the tap's shape is read; `device` names the parameters' device when the tap is a shape-only
    stand-in.  The first block runs at the tap's extent, the others at that divided by the stride."""
    cin, width, stride = stage.cin, stage.width, stage.stride
    blocks = list(layer) if isinstance(layer, (nn.Sequential, list, tuple)) else []
    if len(blocks) != stage.blocks or not all(isinstance(b, Bottleneck) for b in blocks):
        raise RuntimeError(stage.built)
    checks = [_bottleneck_check(b, stage.geometries, stage.family_built) for b in blocks]
    if not torch.is_tensor(tap) or tap.dim() != 4:
        raise RuntimeError(stage.built)
    n, h, w = int(tap.shape[0]), int(tap.shape[1]) - 2, int(tap.shape[2]) - 2
    if ([c[0] for c in checks] != [(cin, width, stride)] + [(4 * width, width, 1)] * (stage.blocks - 1) or tap.shape[3] != cin or
            h < stride or w < stride or h % stride or w % stride or len({c[1] for c in checks}) > 1):
        raise RuntimeError(stage.built)
    ops = [_bottleneck_operands(b, tap.device if device is None else device, stage.geometries, stage.family_built) for b in blocks]
    geoms = [(n, h, w, cin, width, stride)] + [(n, h // stride, w // stride, 4 * width, width, 1)] * (stage.blocks - 1)
    return blocks, geoms, checks[0][1], [o[2] for o in ops], [tuple(o[3]) for o in ops]


def _forward_res_padded(stage, layer, tap):
    if not torch.is_tensor(tap) or tap.dim() != 4:
        raise ValueError("padded taps must be contiguous float16 CUDA tensors [n,h+2,w+2,C]")
    _, geoms, eps, learn, stats = _res_operands(stage, layer, tap)
    _check_padded_taps([tap])
    with torch.no_grad():
        x = tap.detach()
        for g, lr, st in zip(geoms, learn, stats):
            x = _block_forward_raw(x, g, eps, [t.detach() for t in lr], st, stage.entry)[0]
        return x


def forward_res5_padded(layer, c4_tap):
    """ResNet-50's last stage (res5: three Bottlenecks) on a padded C4 tap with the HIP training kernels, no gradient: padded C5
    [n,h5+2,w5+2,2048] fp16 with a zero ring."""
    return _forward_res_padded(_RES_STAGES[3], layer, c4_tap)


def forward_res4_padded(layer, c3_tap):
    """ResNet-50's res4 (six Bottlenecks of width 256) on a padded C3 tap with the HIP training kernels, no gradient: padded C4
    [n,h4+2,w4+2,1024] fp16 with a zero ring."""
    return _forward_res_padded(_RES_STAGES[2], layer, c3_tap)


def forward_res3_padded(layer, c2_tap):
    """ResNet-50's res3 (four Bottlenecks of width 128) on a padded C2 tap with the HIP training kernels, no gradient: padded C3
    [n,h3+2,w3+2,512] fp16 with a zero ring."""
    return _forward_res_padded(_RES_STAGES[1], layer, c2_tap)


def forward_res2_padded(layer, pool_tap):
    """ResNet-50's res2 (three Bottlenecks of width 64) on a padded pooled tap [n,h+2,w+2,64] (the stem's output, e.g.
    DetectorEngine.forward_pool) with the HIP training kernels, no gradient: padded C2 [n,h+2,w+2,256] fp16 with a zero ring."""
    return _forward_res_padded(_RES_STAGES[0], layer, pool_tap)


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
    """Same parameters as text_detector.py:31-41, in the wiring of SURVEY.md B.3 (the one the engine implements):
    L5 = inner_blocks[0](C5), L(k) = inner_blocks[5-k](C(k)) + nearest-2x(L(k+1)), P2 = layer_blocks[3](L2).

    ``fpn([C2, C3, C4, C5])`` on CUDA NCHW tensors (fp32 or fp16; C(k) has in_channels >> (5 - k) channels and each level is exactly twice
    the size of the one above) returns P2 as ``[n,256,H,W]`` fp32 from the HIP training kernels (csrc/fpn_train.hip), differentiable
    w.r.t. the ten live tensors (the four laterals and layer_blocks[3], weights and biases).  layer_blocks[0..2] are dead
    (text_detector.py:56) and receive no gradient, as under torch autograd.  Features that require grad are refused unless the call says
    ``input_grad=True``: then the backward also forms dC(k) = inner_blocks[5-k].weight^T dL(k) for the features that require grad (one
    more GEMM per level, none for the others) and each receives it in its own layout and dtype.  The ten parameter gradients are the same
    bits either way."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.inner_blocks = nn.ModuleList(nn.Conv2d(in_channels >> i, 256, 1) for i in range(4))
        self.layer_blocks = nn.ModuleList(nn.Conv2d(256, 256, 3, padding=1) for _ in range(4))

    def live_parameters(self):
        """The ten tensors that receive a gradient, in the kernels' order."""
        return ([m.weight for m in self.inner_blocks] + [m.bias for m in self.inner_blocks] +
                [self.layer_blocks[3].weight, self.layer_blocks[3].bias])

    def _in_channels(self):
        return self.inner_blocks[0].weight.shape[1]

    def _geometry(self, shapes):
        """(n, h5, w5, c5) from the four (n, C, H, W) shapes C2..C5, or ValueError."""
        c5 = self._in_channels()
        if c5 < 512 or c5 > 4096 or c5 % 512:
            raise ValueError(f"the HIP FPN kernels need in_channels to be a multiple of 512 up to 4096, got {c5}")
        n, _, h5, w5 = shapes[3]
        for lv, shp in enumerate(shapes):
            k = 3 - lv
            if shp[1] != c5 >> k:
                raise ValueError(f"FPN input C{lv + 2} must have {c5 >> k} channels, got {shp[1]}")
            if shp[0] != n or shp[2] != h5 << k or shp[3] != w5 << k:
                raise ValueError(f"FPN inputs must be exact doublings of C5 ({n}x{h5}x{w5}): C{lv + 2} must be [{n},{c5 >> k},{h5 << k},"
                                 f"{w5 << k}], got {list(shp)}")
        if n < 1 or h5 < 1 or w5 < 1:
            raise ValueError("FPN inputs must not be empty")
        return int(n), int(h5), int(w5), int(c5)

    def _live_checked(self, device):
        params = self.live_parameters()
        for t in params:
            if not t.is_cuda or t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("FeaturePyramidNetwork parameters must be contiguous float32 CUDA tensors on the features' device "
                                 "(call .cuda() on the model)")
        return params

    def forward(self, features, input_grad=False):
        if not isinstance(features, (list, tuple)) or len(features) != 4 or not all(torch.is_tensor(t) and t.dim() == 4 for t in features):
            raise ValueError("FeaturePyramidNetwork input must be the four [n,C,H,W] trunk taps [C2, C3, C4, C5]")
        geom = self._geometry([tuple(t.shape) for t in features])
        if any(t.requires_grad for t in features) and not input_grad:
            raise RuntimeError("FeaturePyramidNetwork: the input features require grad, but backward into the trunk is not built; "
                               "only the FPN's own parameters receive a gradient (pass features.detach(), or input_grad=True for the "
                               "gradient of the features themselves)")
        if not all(t.is_cuda for t in features):
            raise ValueError("FeaturePyramidNetwork runs on the HIP kernels: features must be CUDA (HIP) tensors")
        params = self._live_checked(features[0].device)
        srcs = [t if input_grad and t.requires_grad and torch.is_grad_enabled() else None for t in features]
        return _FPNTrainFn.apply(tuple(pack_tap(t) for t in features), geom, *srcs, *params)

    def forward_padded(self, taps, head=None, layer4=None, layer3=None, layer2=None, layer1=None, stem=None, trunk_batch_stats=False,
                       stem_batch_stats=False, res5=None, res4=None, res3=None, res2=None, res_batch_stats=False):
        """`res_batch_stats` (True, or the tuple of exactly the res stages given: ("res5",) or ("res4", "res5")) goes with `res5`, a DBHead and
        the taps [C2, C3, C4], or with `res4`, `res5`, a DBHead and the taps [C2, C3]: the res5 -> FPN -> head node or the res4 -> res5 -> FPN ->
        head node described below with every Bottleneck on the vtd_bottleneck_bn_train_* entries (csrc/bottleneck_bn_train.hip), so the
        stages' BatchNorms behave as torch's do in the mode they are in: in train() mode the statistics of the batch normalise, the running
        statistics are updated in place and num_batches_tracked advances (10 BatchNorms for res5, 29 with res4); in eval() mode the frozen
        path runs, the same bits as without the keyword.  The three or nine blocks must be in one mode with one fixed momentum and one eps.
        The parameter gradients of a block do not depend on whether its input gradient is formed, so the res5 node gives the bits of the
        deeper node's res5 gradients when fed the taps that node produced.  With `res3`, `res2`, `stem`, any ResNet-18 argument, without
        `res5` or without a head it raises ValueError before a device is looked at: res3, res2 and the stem keep frozen statistics.

        `res2` (ResNet-50's res2, an nn.Sequential of three Bottlenecks of width 64) goes with `res3`, `res4`, `res5`, a DBHead and the padded
        pooled tap [pool] of 64 channels and extents that are multiples of 8 (C2 .. C5 are computed here): res2 -> res3 -> res4 -> res5 -> FPN
        -> head as ONE autograd node of sixteen blocks, per = (3, 4, 6, 3), res2 on the vtd_bottleneck64_train_* entries, differentiable
        w.r.t. res2's thirty learnable tensors and the 156 above.  C2 .. C5 are the outputs of blocks 3, 7, 13 and 16; the FPN forms dC2 ..
        dC5; res3.0's strided input gradient is added to the FPN's dC2 once, at one power-of-two scale; res2.0 forms no input gradient.
        With `stem=(conv, bn)` too, on the tap [image] (nets.pack_image): stem -> res2 -> .. -> head, the stem on the frozen-statistics
        vtd_stem_train_* entries, and res2.0's input gradient is the stem's dpool.  Without `res3`, `res4` and `res5`, without a head, or
        with a ResNet-18 stage argument or batch-statistics flag it raises ValueError.

        `res3` (ResNet-50's res3, an nn.Sequential of four Bottlenecks of width 128) goes with `res4`, `res5`, a DBHead and the padded tap [C2]
        of 256 channels and extents that are multiples of 8 (further entries are ignored: C3, C4 and C5 are computed here): res3 -> res4 ->
        res5 -> FPN -> head as ONE autograd node, res3 on the vtd_bottleneck128_train_* entries, differentiable w.r.t. res3's thirty-nine
        learnable tensors, res4's fifty-seven, res5's thirty, the FPN's ten and the head's twenty.  C3 is the fourth block's output, C4 the
        tenth's and C5 the thirteenth's; the FPN forms dC5, dC4 and dC3; res5's and res4's first blocks form their strided input gradients,
        each added to the FPN's gradient of that level once, at one power-of-two scale; res3's blocks 3 .. 1 form their input gradients,
        block 0 forms none (no dC2).  Without `res4` and `res5`, without a head, or with a ResNet-18 stage argument or batch-statistics flag
        it raises ValueError.

        `res4` (ResNet-50's res4, an nn.Sequential of six Bottlenecks of width 256) goes with `res5`, a DBHead and the padded taps [C2, C3] of
        256 and 512 channels (further entries are ignored: C4 and C5 are computed here): res4 -> res5 -> FPN -> head as ONE autograd node, res4
        on the vtd_bottleneck256_train_* entries and res5 on vtd_bottleneck_train_* (csrc/bottleneck_train.hip, frozen-statistics BatchNorm),
        differentiable w.r.t. res4's fifty-seven learnable tensors, res5's thirty, the FPN's ten and the head's twenty.  C4 is the sixth
        block's output and C5 the ninth's; the FPN forms dC5 and dC4; res5's first block forms its strided input gradient, which is added to
        the FPN's dC4 at one power-of-two scale; res4's blocks 5 .. 1 form their input gradients, block 0 forms none (no dC3).  Without
        `res5`, without a head, or with a ResNet-18 stage argument or batch-statistics flag it raises ValueError.

        `res5` (ResNet-50's last stage, an nn.Sequential of three Bottlenecks of width 512) goes with a DBHead and the padded taps [C2, C3, C4]
        of 256, 512 and 1024 channels (a fourth entry is ignored: C5 is computed here from C4): res5 -> FPN -> head as ONE autograd node on the
        vtd_bottleneck_train_* entries (csrc/bottleneck_train.hip, frozen-statistics BatchNorm), differentiable w.r.t. the stage's thirty
        learnable tensors, the FPN's ten and the head's twenty.  dC5 goes into the last block as the FPN leaves it; blocks 2 and 1 form their
        input gradients, block 0 forms none.  With `layer1` .. `layer4`, `stem`, `trunk_batch_stats` or `stem_batch_stats`, or without a head,
        it raises ValueError.

        `stem_batch_stats=True` goes with `stem`, `layer1` .. `layer4`, `head`, `trunk_batch_stats=("layer1", "layer2", "layer3", "layer4")` and
        the tap [image]: the stem -> layer1 -> .. -> layer4 -> FPN -> head node with the stem on the vtd_stem_bn_train_* entries and the eight
        blocks on vtd_trunk_bn_train_*, so every BatchNorm of the trunk behaves as torch's does in the mode it is in.  The stem's BatchNorm
        must be in the mode of the eight blocks and keeps its own eps and momentum; anything else raises ValueError before the device is looked
        at.  The other eighty-seven gradients and the stages' buffers are the bits of the four-stage batch node below on the pooled tap the
        stem wrote.  Without the keyword every call behaves as before.

        `trunk_batch_stats=("layer1", "layer2", "layer3", "layer4")` goes with the tap [pool], `layer1` .. `layer4` and `head` and no `stem`:
        the layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head node with all eight blocks on the vtd_trunk_bn_train_* entries, in one mode with
        one momentum and one eps, else ValueError before the device is looked at.  layer2.0, layer3.0 and layer4.0 form their input gradients
        (dC2 is layer2.0's plus the FPN's dC2, as in the frozen layer1 node); layer1.0 forms none.

        `trunk_batch_stats=("layer2", "layer3", "layer4")` goes with the tap [C2], `layer2`, `layer3`, `layer4` and `head` and nothing lower:
        the layer2 -> layer3 -> layer4 -> FPN -> head node with all six blocks on the vtd_trunk_bn_train_* entries, in one mode (train() or
        eval()) with one momentum and one eps, else ValueError before the device is looked at.  layer3.0 and layer4.0 form their input
        gradients (dC3 and dC4 are those plus the FPN's); layer2.0 forms none.

        `trunk_batch_stats` may also be a tuple or list of stage names.  ("layer4",) means what True means.  ("layer3", "layer4") goes with
        taps [C2, C3], `layer3`, `layer4` and `head` and nothing lower: the four blocks run on the vtd_block_bn_train_* entries, in one mode
        (train() or eval()) with one momentum and one eps, else ValueError; layer4.0 forms its input gradient (dz1 through the strided dgrad
        plus the downsample's transpose of its own dz), which is combined with the FPN's dC4; layer3.0 forms none.  Any other tuple raises
        ValueError.

        With `trunk_batch_stats=True` (the layer4 -> FPN -> head node only: passing it with `layer3` or a lower stage raises ValueError)
        layer4 runs on the vtd_resblock_bn_train_* entries: while layer4 is in training mode its five BatchNorms normalise with the statistics
        of the batch, their running statistics are updated in place and their num_batches_tracked advance; in eval() mode the frozen path
        runs, the same bits as without the flag.

        With `stem` too (the pair (conv 7x7/s2, BatchNorm) of ResNet's stem): stem -> layer1 -> .. -> layer4 -> FPN -> head as ONE autograd
        node on the image tap [image] (nets.pack_image: [n,H+6,W+6,4] fp16), differentiable w.r.t. the stem's three learnable tensors and the
        eighty-seven below.  layer1.0 forms its input gradient and that gradient is the stem's dpool; the other eighty-seven gradients are the
        bits of the node without `stem` on the pooled tap the stem produced.  No gradient of the image is formed.

        With `layer1` too (ResNet-18's first stage, two 64 -> 64 BasicBlocks): layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head as ONE
        autograd node on the padded tap [pool] (the pooled stem output, e.g. DetectorEngine.forward_pool; C2..C5 are computed here),
        differentiable w.r.t. layer1's twelve learnable tensors, the forty-five of the three stages above, the FPN's ten and the head's
        twenty.  dC2 is layer2.0's input gradient (the strided dgrad) plus the FPN's dC2; layer1.0 forms no input gradient.

        With `layer2` too (ResNet-18's second stage): layer2 -> layer3 -> layer4 -> FPN -> head as ONE autograd node on the padded tap [C2]
        (further entries are ignored: C3, C4 and C5 are computed here), differentiable w.r.t. the forty-five learnable tensors of the three
        stages, the FPN's ten and the head's twenty.  dC3 is layer3.0's input gradient plus the FPN's dC3, dC4 as below; layer2.0 forms no
        input gradient.

        With `layer3` (ResNet-18's third stage, two BasicBlocks): layer3 -> layer4 -> FPN -> head as ONE autograd node on the padded taps
        [C2, C3] (further entries are ignored: C4 and C5 are computed here), differentiable w.r.t. the thirty learnable tensors of the two
        stages, the FPN's ten and the head's twenty.  dC4 is layer4.0's input gradient plus the FPN's dC4, added at one power-of-two scale.

        With `layer4` (ResNet-18's last stage, an nn.Sequential of two BasicBlocks) and a DBHead: layer4 -> FPN -> head as ONE autograd node
        on the padded taps [C2, C3, C4] (a fourth entry is ignored: C5 is computed here from C4), differentiable w.r.t. layer4's fifteen
        learnable tensors, the FPN's ten and the head's twenty; dP2 and dC5 travel between the stages as the kernels leave them (NHWC fp32
        with their power-of-two scales), never through fp16.  Otherwise:

        The FPN on padded taps (ring-padded NHWC fp16 [n,h+2,w+2,C] for C2..C5, e.g. DetectorEngine.forward_trunk).  Without `head`:
        P2 as padded features (what DBHead.forward_padded reads), no gradient.  With a DBHead: FPN -> head as ONE autograd node that
        returns the head's maps, differentiable w.r.t. the FPN's ten live tensors and the head's twenty; the head's input gradient goes
        to the FPN's backward as the kernels leave it (NHWC fp32 with its power-of-two scale), never through an fp16 tensor."""
        layers, res = (layer1, layer2, layer3, layer4), (res2, res3, res4, res5)
        if res_batch_stats:
            given = tuple(k for k, m in (("res4", res4), ("res5", res5)) if m is not None)
            if res5 is None or res3 is not None or res2 is not None or stem is not None or any(m is not None for m in layers) or \
                    trunk_batch_stats or stem_batch_stats or head is None:
                raise ValueError(f"forward_padded(..., res_batch_stats={res_batch_stats!r}) is the res5 -> FPN -> head node on the taps [C2, C3, C4] "
                                 "or the res4 -> res5 -> FPN -> head node on the taps [C2, C3]: it needs res5 and the head and takes no res3, "
                                 "res2, stem, layer1 .. layer4, trunk_batch_stats or stem_batch_stats; " + _RES_BN_BUILT)
            if res_batch_stats is not True and not (isinstance(res_batch_stats, (tuple, list)) and tuple(res_batch_stats) == given):
                raise ValueError(f"forward_padded(..., res_batch_stats={res_batch_stats!r}) must be True or the tuple of exactly the res stages "
                                 f"given, {given!r}; " + _RES_BN_BUILT)
            return self._forward_padded_res(taps, head, res, None, batch=True)
        if any(m is not None for m in res):      # ResNet-50's node, from the lowest stage given up
            low = next(i for i, m in enumerate(res) if m is not None)
            names = [st.name for st in _RES_STAGES[low:]]
            node = " -> ".join(names) + " -> FPN -> head node"
            spelled = ", ".join(f"{name}=..." for name in reversed(names))
            if any(m is None for m in res[low:]):
                raise ValueError(f"forward_padded(taps, head=head, {names[0]}=...) is ResNet-50's {node}: it needs {_listed(names[1:])} too")
            if any(m is not None for m in layers) or (stem is not None and low > 0) or trunk_batch_stats or stem_batch_stats:      # res2 takes the stem
                raise ValueError(f"forward_padded(taps, head=head, {spelled}) is ResNet-50's {node} with frozen-statistics BatchNorm: it takes no "
                                 f"layer1 .. layer4, {'stem, ' if low > 0 else ''}trunk_batch_stats or stem_batch_stats (those are ResNet-18's)")
            if head is None:
                raise ValueError(f"forward_padded(taps, {spelled}) is the training node: it needs the DBHead too")
            return self._forward_padded_res(taps, head, res, stem)
        if stem_batch_stats:
            return self._forward_padded_batch_stem(taps, head, layers, stem, trunk_batch_stats, stem_batch_stats)
        bn_stages = ()
        if isinstance(trunk_batch_stats, (tuple, list)):
            bn_stages = tuple(trunk_batch_stats)
            if not any(bn_stages == stages for stages in _NODE_BN_STAGES):      # no hashing: any tuple may come
                raise ValueError(f"forward_padded(..., trunk_batch_stats={trunk_batch_stats!r}): " + _TRUNK_BN_BUILT)
        elif trunk_batch_stats:
            bn_stages = ("layer4",)
        if bn_stages == ("layer4",) and (layer4 is None or any(m is not None for m in (layer3, layer2, layer1, stem))):
            raise ValueError("forward_padded(..., trunk_batch_stats=True) is the layer4 -> FPN -> head node: " + _BN_TRAIN_BUILT)
        if len(bn_stages) == 2 and (layer4 is None or layer3 is None or any(m is not None for m in (layer2, layer1, stem))):
            raise ValueError("forward_padded(..., trunk_batch_stats=('layer3', 'layer4')) is the layer3 -> layer4 -> FPN -> head node on the taps "
                             "[C2, C3]: it needs layer3, layer4 and the head and takes no lower stage; " + _TRUNK_BN_BUILT)
        if len(bn_stages) == 3 and (layer4 is None or layer3 is None or layer2 is None or layer1 is not None or stem is not None):
            raise ValueError("forward_padded(..., trunk_batch_stats=('layer2', 'layer3', 'layer4')) is the layer2 -> layer3 -> layer4 -> FPN -> head "
                             "node on the tap [C2]: it needs layer2, layer3, layer4 and the head and takes no lower stage; " + _TRUNK_BN_BUILT)
        if len(bn_stages) == 4 and (any(m is None for m in layers) or stem is not None):
            raise ValueError("forward_padded(..., trunk_batch_stats=('layer1', 'layer2', 'layer3', 'layer4')) is the layer1 -> layer2 -> layer3 -> "
                             "layer4 -> FPN -> head node on the tap [pool]: it needs layer1, layer2, layer3, layer4 and the head and takes no stem, "
                             "which keeps frozen statistics; " + _TRUNK_BN_BUILT)
        if stem is not None or any(m is not None for m in layers):
            return self._forward_padded_trunk(taps, head, layers, stem, bn_stages)
        if not isinstance(taps, (list, tuple)) or len(taps) != 4:
            raise ValueError("padded taps must be the four tensors [C2, C3, C4, C5]")
        _check_padded_taps(taps)
        geom = self._geometry([_tap_nchw(t) for t in taps])
        params = self._live_checked(taps[0].device)
        taps = tuple(t.detach() for t in taps)
        if head is None:
            return _fpn_forward_raw(taps, geom, [p.detach() for p in params])[0]
        bns, hparams, hbuffers = head._train_operands(taps[0].device)
        plan = _TrunkPlan(taps, geom, (head.training, bns[0].momentum, bns[0].eps, tuple(hbuffers)), None, (), None, None)      # no trunk stage
        return self._run_node(head, bns, plan, *params, *hparams)

    @staticmethod
    def _res_bn_plan(layers, c5):
        """The batch-statistics plan of a res node: (the blocks' BatchNorms, (training, momentum)), judged without looking at any device."""
        blocks = [b for layer in layers for b in layer]
        checks = [_bottleneck_bn_check(b) for b in blocks]
        bbns = [bn for c in checks for bn in c[2]]
        if any(b.training != blocks[0].training for b in blocks) or any(c[3] != checks[0][3] for c in checks):
            raise ValueError(f"the {len(blocks)} Bottlenecks of a res_batch_stats node must be in one mode (train() or eval()) with one fixed "
                             "BatchNorm momentum")
        n, _, h5, w5 = c5
        if blocks[0].training and n * h5 * w5 < 2:
            raise ValueError(f"train-mode BatchNorm needs more than one value per channel, got a C5 of {n} x {h5} x {w5}")
        return bbns, (bool(blocks[0].training), checks[0][3])

    def _forward_padded_res(self, taps, head, layers, stem, batch=False):
        """forward_padded with ResNet-50 stages: `layers` is (res2, res3, res4, res5) with None below the lowest one given, where the node
        starts (with `stem`, which goes with res2: at the stem, on the image tap).  `batch`: every block on the vtd_bottleneck_bn_train_*
        entries, the blocks' mode deciding between batch and frozen statistics."""
        low = next(i for i, m in enumerate(layers) if m is not None)
        # the taps the node reads: the FPN levels below the lowest stage's output, the last of them that stage's input; res2 reads the pooled
        # stem output and the stem the image, neither an FPN level
        names = ["image"] if stem is not None else [st.tap for st in _RES_STAGES[1:low + 1]] or [_RES_STAGES[0].tap]
        if not isinstance(taps, (list, tuple)) or len(taps) < len(names):
            raise ValueError(f"padded taps must be the tensors [{', '.join(names)}]")
        if stem is not None and (not isinstance(stem, (list, tuple)) or len(stem) != 2):
            raise ValueError("stem must be the pair (conv, bn) of the trunk's first two modules")
        taps = tuple(t.detach() if torch.is_tensor(t) else t for t in taps[:len(names)])
        slearn, splan = [], None
        if stem is None:
            _check_padded_taps(taps)
            x = taps[-1]
        else:
            sgeom, seps, slearn, sstats = _stem_operands(stem[0], stem[1], taps[0])
            splan = (sgeom, seps, tuple(sstats))
            x = _meta_tap(sgeom[0], (sgeom[1] // 2 + 1) // 2, (sgeom[2] // 2 + 1) // 2, 64)
        dev = taps[-1].device
        stages, ops, outs = _RES_STAGES[low:], [], []      # per stage: _res_operands' result, and its output C(k) as (n, C, h, w)
        for st, layer in zip(stages, layers[low:]):      # every stage above the lowest is judged on a stand-in of the shape the one below gives
            ops.append(_res_operands(st, layer, x, dev))
            n, h, w = ops[-1][1][-1][:3]      # the extent the stage's last block runs at
            if st.name == "res2" and (h % 8 or w % 8):      # C5 is an eighth of the pooled tap
                raise RuntimeError(_RES2_BUILT + f"; the node needs a pooled tap whose extents are multiples of 8, got {h} x {w}")
            outs.append((n, 4 * st.width, h, w))
            x = _meta_tap(n, h, w, 4 * st.width)
        beps = ops[0][2]
        if any(o[2] != beps for o in ops):
            raise ValueError("the HIP Bottleneck kernels need one eps on all BatchNorms of " + _listed([st.name for st in stages]))
        geom = self._geometry(([_tap_nchw(t) for t in taps] + outs)[-4:])      # C2 .. C5: the last four (the image and the pooled tap fall out)
        params = self._live_checked(dev)
        bns, hparams, hbuffers = head._train_operands(dev)
        bbns, bn = self._res_bn_plan(layers[low:], outs[-1]) if batch else ([], None)
        blocks = tuple(_BlockPlan(g, s, _BOTTLENECK_BN if batch else st.entry, len(lr))
                       for st, (_, geoms, _, learn, stats) in zip(stages, ops) for g, lr, s in zip(geoms, learn, stats))
        per = 3 if len(stages) == 1 else tuple(st.blocks for st in stages)      # res5 alone: every stage has three
        plan = _TrunkPlan(taps, geom, (head.training, bns[0].momentum, bns[0].eps, tuple(hbuffers)), splan, blocks, beps, bn, per)
        out = self._run_node(head, bns, plan, *slearn, *(t for o in ops for lr in o[3] for t in lr), *params, *hparams)
        if bn is not None and bn[0]:
            with torch.no_grad():
                for b in bbns:
                    b.num_batches_tracked.add_(1)
        return out

    def _forward_padded_batch_stem(self, taps, head, layers, stem, trunk_batch_stats, stem_batch_stats):
        """forward_padded(..., stem_batch_stats=True): the whole-backbone node with batch statistics in the stem too."""
        node = ("forward_padded(..., stem=(conv, bn), trunk_batch_stats=('layer1', 'layer2', 'layer3', 'layer4'), stem_batch_stats=True) is the "
                "stem -> layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head node with batch statistics in all twenty BatchNorms of the trunk")
        if stem_batch_stats is not True:
            raise ValueError(node + f": stem_batch_stats is True or False, got {stem_batch_stats!r}")
        if not isinstance(trunk_batch_stats, (tuple, list)) or tuple(trunk_batch_stats) != _NODE_BN_STAGES[3]:
            raise ValueError(node + f": it takes the four-stage tuple, got trunk_batch_stats={trunk_batch_stats!r}")
        if head is None or any(m is None for m in layers) or not isinstance(stem, (list, tuple)) or len(stem) != 2:
            raise ValueError(node + ": it needs stem (the pair (conv, bn) of the trunk's first two modules), layer1, layer2, layer3, layer4 and the head")
        sbn = stem[1]
        bnm = [m for layer in layers for m in layer.modules() if isinstance(m, nn.BatchNorm2d)]
        if isinstance(sbn, nn.BatchNorm2d):
            if sbn.momentum is None:
                raise ValueError(_STEM_BN_MOMENTUM)
            if any(m.training != sbn.training for m in bnm):
                raise ValueError(node + ": the stem's BatchNorm must be in the mode (train() or eval()) of the eight blocks")
        return self._forward_padded_trunk(taps, head, layers, stem, _NODE_BN_STAGES[3], stem_bn=True)

    @staticmethod
    def _run_node(head, bns, plan, *learn):
        prob, thresh, _ = _TrunkFPNHeadTrainFn.apply(plan, *learn)
        head._batches_seen(bns)
        return {"probability": prob, "threshold": thresh}

    def _forward_padded_trunk(self, taps, head, layers, stem, bn_stages, stem_bn=False):
        """forward_padded with trunk stages: `layers` is (layer1, layer2, layer3, layer4), the node starts at the lowest one given (with `stem`:
        at the stem) and needs every stage above it and the head.  `bn_stages`: () or the stages (all of the node's) that run with batch
        statistics, ("layer4",) on the vtd_resblock_bn_train_* entries, ("layer3", "layer4") on vtd_block_bn_train_*, ("layer2", "layer3",
        "layer4") or ("layer1", "layer2", "layer3", "layer4") on vtd_trunk_bn_train_*.  `stem_bn`: the stem on the vtd_stem_bn_train_* entries (with
        the four-stage tuple only: _forward_padded_batch_stem)."""
        low = 0 if stem is not None else next(i for i, m in enumerate(layers) if m is not None)
        above = _STAGES[0 if stem is not None else low + 1:]
        if head is None or any(m is None for m in layers[4 - len(above):]):
            raise ValueError(f"forward_padded(taps, {'stem' if stem is not None else _STAGES[low].name}=...) is the training node: it needs "
                             + ", ".join(st.name for st in above) + (" and " if above else "") + "the DBHead too")
        if stem is not None and (not isinstance(stem, (list, tuple)) or len(stem) != 2):
            raise ValueError("stem must be the pair (conv, bn) of the trunk's first two modules")
        if len(bn_stages) == 2:      # the plan is node-wide: one eps over the four blocks (one mode and one momentum are checked below)
            eps_all = {m.eps for layer in layers[2:] for m in layer.modules() if isinstance(m, nn.BatchNorm2d)}
            if len(eps_all) > 1:
                raise ValueError("layer3's and layer4's four blocks must have one BatchNorm eps")
        if len(bn_stages) >= 3:      # the same over the six or eight blocks, with the mode and the momentum: all before the device is looked at
            bnm = [m for layer in layers[4 - len(bn_stages):] for m in layer.modules() if isinstance(m, nn.BatchNorm2d)]
            whose = "layer2's, layer3's and layer4's six" if len(bn_stages) == 3 else "layer1's, layer2's, layer3's and layer4's eight"
            if len({m.eps for m in bnm}) > 1:
                raise ValueError(whose + " blocks must have one BatchNorm eps")
            if len({m.training for m in bnm}) > 1 or any(m.momentum is None or m.momentum != bnm[0].momentum for m in bnm):
                raise ValueError(whose + " blocks must be in one mode (train() or eval()) with one fixed BatchNorm momentum")
        # the taps the node reads: the FPN levels below the lowest stage's output, the last of them that stage's input; layer1 reads the pooled
        # stem output and the stem the image, neither an FPN level
        names = ["image"] if stem is not None else [st.tap for st in _STAGES[1:low + 1]] or [_STAGES[0].tap]
        if not isinstance(taps, (list, tuple)) or len(taps) < len(names):
            raise ValueError(f"padded taps must be the tensor{'s' if len(names) > 1 else ''} [{', '.join(names)}]")
        taps = tuple(t.detach() if torch.is_tensor(t) else t for t in taps[:len(names)])
        slearn, splan = [], None
        if stem is None:
            _check_padded_taps(taps)
            x = taps[-1]
        else:
            sgeom, seps, slearn, sstats = _stem_operands(stem[0], stem[1], taps[0])
            splan = (sgeom, seps, tuple(sstats)) + ((_stem_bn_plan(stem[1], sgeom),) if stem_bn else ())
            x = _meta_tap(sgeom[0], (sgeom[1] // 2 + 1) // 2, (sgeom[2] // 2 + 1) // 2, 64)
        dev = taps[-1].device
        ops, outs = [], []      # per stage: _stage_operands' result, and its output C(k) as (n, C, h, w)
        for st, layer in zip(_STAGES[low:], layers[low:]):      # each stage's output shape is the next one's input
            ops.append(_stage_operands(st, layer, x, dev))
            n, h, w = ops[-1][1][1][:3]      # the extent the stage's second block runs at
            outs.append((n, st.width, h, w))
            x = _meta_tap(n, h, w, st.width)
        beps = ops[0][2]
        if any(o[2] != beps for o in ops):
            raise RuntimeError(" / ".join(st.name for st in _STAGES[low:]) + " training needs one BatchNorm eps")
        geom = self._geometry(([_tap_nchw(t) for t in taps] + outs)[-4:])      # C2 .. C5: the last four (the image and the pooled tap fall out)
        params = self._live_checked(dev)
        bns, hparams, hbuffers = head._train_operands(dev)
        bn, bbns = None, []
        if bn_stages:
            blocks = [blk for o in ops for blk in o[0]]      # the node's stages are exactly bn_stages (forward_padded)
            trunk_check = (_TRUNK_BLOCK_BN_GEOMETRIES, _TRUNK_BLOCK_BN_BUILT)
            check = ((), (_BLOCK_BN_GEOMETRIES, _BLOCK_BN_BUILT), trunk_check, trunk_check)[len(bn_stages) - 1]
            bbns = [b for blk in blocks for b in _block_bn_check(blk, *check)]
            if any(blk.training != blocks[0].training for blk in blocks) or any(b.momentum != bbns[0].momentum for b in bbns):
                raise ValueError(("layer4's two", "layer3's and layer4's four", "layer2's, layer3's and layer4's six",
                                  "layer1's, layer2's, layer3's and layer4's eight")[len(bn_stages) - 1] +
                                 " blocks must be in one mode (train() or eval()) with one BatchNorm momentum")
            n, _, h5, w5 = outs[-1]
            if blocks[0].training and n * h5 * w5 < 2:
                raise ValueError(f"train-mode BatchNorm needs more than one value per channel, got a C5 of {n} x {h5} x {w5}")
            bn = (bool(blocks[0].training), float(bbns[0].momentum))
        blocks = []
        for _, geoms, _, learn, stats in ops:
            for g, lr, s in zip(geoms, learn, stats):
                # a node of one stage runs on that stage's own entry family, as forward_<stage>_padded does; a deeper one on the block's by width
                entry = (_RESBLOCK_BN, _BLOCK_BN, _TRUNK_BN, _TRUNK_BN)[len(bn_stages) - 1] if bn is not None else _STAGES[low].entry if len(ops) == 1 else _block_entry(g)
                blocks.append((_BlockPlan(g, s, entry, len(lr)), lr))
        plan = _TrunkPlan(taps, geom, (head.training, bns[0].momentum, bns[0].eps, tuple(hbuffers)), splan, tuple(b for b, _ in blocks), beps, bn)
        out = self._run_node(head, bns, plan, *slearn, *(t for _, lr in blocks for t in lr), *params, *hparams)
        if bn is not None and bn[0]:
            with torch.no_grad():
                for b in bbns:
                    b.num_batches_tracked.add_(1)
        if stem_bn and splan[3][0]:
            with torch.no_grad():
                stem[1].num_batches_tracked.add_(1)
        return out


def _check_padded_taps(taps):
    for t in taps:
        # the kernels trust the buffers' extents: a mismatch here would be a device-side out-of-bounds read
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous() or t.dim() != 4 or t.shape[1] < 3 or t.shape[2] < 3:
            raise ValueError("padded taps must be contiguous float16 CUDA tensors [n,h+2,w+2,C]")


def _tap_nchw(tap):
    """The (n, C, h, w) a padded tap [n,h+2,w+2,C] holds."""
    return (tap.shape[0], tap.shape[3], tap.shape[1] - 2, tap.shape[2] - 2)


def _meta_tap(n, h, w, c):
    """A shape-only stand-in for the padded tap [n,h+2,w+2,c] that a stage of the node will produce."""
    return torch.empty((n, h + 2, w + 2, c), dtype=torch.float16, device="meta")


def _stem_operands(conv, bn, image_tap):
    """ResNet's stem (conv 7x7/s2/p3 3 -> 64 without bias, BatchNorm(64)) on an image tap [n,H+6,W+6,4] fp16: ((n, H, W), eps, the learnable
    tensors [conv.weight, bn.weight, bn.bias], the running statistics (mean, var)), validated."""
    if (not isinstance(conv, nn.Conv2d) or not isinstance(bn, nn.BatchNorm2d) or conv.bias is not None or tuple(conv.weight.shape) != (64, 3, 7, 7)
            or conv.stride != (2, 2) or conv.padding != (3, 3) or conv.dilation != (1, 1) or conv.groups != 1 or bn.num_features != 64
            or not bn.affine or not bn.track_running_stats):
        raise RuntimeError("stem training is built for ResNet's stem: Conv2d(3, 64, 7, stride 2, padding 3, no bias) and BatchNorm2d(64) with "
                           "running statistics")
    t = image_tap
    if (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous() or t.dim() != 4 or t.shape[3] != 4 or t.shape[0] < 1
            or t.shape[1] < 8 or t.shape[2] < 8 or t.shape[1] % 2 or t.shape[2] % 2):
        raise ValueError("the image tap must be a contiguous float16 CUDA tensor [n,H+6,W+6,4] with even H and W (nets.pack_image)")
    learn, stats = [conv.weight, bn.weight, bn.bias], (bn.running_mean, bn.running_var)
    for p in learn + list(stats):
        if not p.is_cuda or p.device != t.device or p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("stem parameters and buffers must be contiguous float32 CUDA tensors on the input's device (call .cuda() on the model)")
    return (int(t.shape[0]), int(t.shape[1]) - 6, int(t.shape[2]) - 6), float(bn.eps), learn, stats


def _stem_struct(learn, stats=None):
    import ctypes as C
    from . import _native
    st = _native.StemParams()
    for field, t in zip(("w", "gamma", "beta"), learn):
        setattr(st, field, C.c_void_p(t.data_ptr()))
    if stats is not None:
        st.mean, st.var = C.c_void_p(stats[0].data_ptr()), C.c_void_p(stats[1].data_ptr())
    return st


def _stem_forward_raw(tap, geom, eps, learn, stats, bn=None, stats_out=None):
    """vtd_stem_train_forward on an image tap: (the pooled padded tap [n,hp+2,wp+2,64] fp16, idx [n,hp,wp,64] uint8, workspace).  With
    `bn` = (training, momentum): vtd_stem_bn_train_forward, which with training set normalises with the statistics of the batch and updates
    `stats` in place; `stats_out` (a float32 CUDA tensor [2,64], optional) then receives the batch's mu and biased sigma^2."""
    n, H, W = geom
    hp, wp = (H // 2 + 1) // 2, (W // 2 + 1) // 2
    query = "vtd_stem_train_workspace_bytes" if bn is None else "vtd_stem_bn_train_workspace_bytes"
    C, _native, lib, ws = _native_workspace(query, (n, H, W, 0), tap.device)
    pool = torch.empty((n, hp + 2, wp + 2, 64), dtype=torch.float16, device=tap.device)
    idx = torch.empty((n, hp, wp, 64), dtype=torch.uint8, device=tap.device)
    st = _stem_struct(learn, stats)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if bn is None:
        _native.check(lib.vtd_stem_train_forward(ptr(tap), n, H, W, C.byref(st), eps, ptr(ws), ptr(pool), ptr(idx), stream), "vtd_stem_train_forward")
    else:
        _native.check(lib.vtd_stem_bn_train_forward(ptr(tap), n, H, W, C.byref(st), int(bn[0]), bn[1], eps, ptr(ws), ptr(pool), ptr(idx),
                                                    None if stats_out is None else ptr(stats_out), stream), "vtd_stem_bn_train_forward")
    return pool, idx, ws


def _stem_backward_raw(tap, geom, eps, learn, stats, ws, pool, idx, dpool, dscale, bn=None):
    """vtd_stem_train_backward (with `bn` = (training, momentum): vtd_stem_bn_train_backward) on dpool as NHWC fp32 [n,hp,wp,64] times
    dscale[0]: the gradients of [conv.weight, bn.weight, bn.bias]."""
    n, H, W = geom
    grads = [torch.empty_like(p) for p in learn]
    query = "vtd_stem_train_workspace_bytes" if bn is None else "vtd_stem_bn_train_workspace_bytes"
    C, _native, lib, scratch = _native_workspace(query, (n, H, W, 1), tap.device)
    st, gst = _stem_struct(learn, stats), _stem_struct(grads)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if bn is None:
        _native.check(lib.vtd_stem_train_backward(ptr(tap), n, H, W, C.byref(st), eps, ptr(ws), ptr(pool), ptr(idx), ptr(dpool), ptr(dscale), C.byref(gst),
                                                  ptr(scratch), stream), "vtd_stem_train_backward")
    else:
        _native.check(lib.vtd_stem_bn_train_backward(ptr(tap), n, H, W, C.byref(st), int(bn[0]), eps, ptr(ws), ptr(pool), ptr(idx), ptr(dpool), ptr(dscale),
                                                     C.byref(gst), ptr(scratch), stream), "vtd_stem_bn_train_backward")
    return grads


class _StemTrainFn(torch.autograd.Function):
    """The stem on the HIP training kernels (csrc/stem_train.hip): image tap in, the pooled map [n,64,hp,wp] fp32 out, differentiable w.r.t.
    the convolution's weight and the BatchNorm's gamma and beta.  No gradient of the image is formed.  `bn`: None (vtd_stem_train_*) or
    (training, momentum) for the vtd_stem_bn_train_* entries."""

    @staticmethod
    def forward(ctx, tap, geom, eps, stats, bn, *learn):
        pool, idx, ws = _stem_forward_raw(tap, geom, eps, learn, stats, bn)
        ctx.save_for_backward(tap, pool, idx, *stats, *learn)
        ctx.ws, ctx.geom, ctx.eps, ctx.bn = ws, geom, eps, bn
        return pool[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        tap, pool, idx, mean, var, *learn = ctx.saved_tensors
        dpool = grad_out.to(torch.float32).permute(0, 2, 3, 1).contiguous()
        dscale = torch.ones(2, dtype=torch.float32, device=dpool.device)
        grads = _stem_backward_raw(tap, ctx.geom, ctx.eps, learn, (mean, var), ctx.ws, pool, idx, dpool, dscale, ctx.bn)
        return (None, None, None, None, None, *grads)


def pack_image(x):
    """[n,3,H,W] float32 / float16 CUDA tensor (H and W even) -> the stem's input layout on the device: ring-padded NHWC fp16 [n,H+6,W+6,4]
    with ring 3, a zero fourth channel and a zero ring."""
    import ctypes as C
    from . import _native
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("the stem's input must be a [n,3,H,W] tensor")
    if not x.is_cuda:
        raise ValueError("the stem runs on the HIP kernels: the input must be a CUDA (HIP) tensor")
    lib = _native.require()
    x = x.detach()
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = x.contiguous()
    n, _, H, W = x.shape
    if n < 1 or H < 2 or W < 2 or H % 2 or W % 2:
        raise RuntimeError(f"the stem's HIP training kernels need a non-empty input with even extents, got {tuple(x.shape)}")
    out = torch.empty((n, H + 6, W + 6, 4), dtype=torch.float16, device=x.device)
    _native.check(lib.vtd_stem_train_pack_input(C.c_void_p(x.data_ptr()), 0 if x.dtype == torch.float32 else 1, n, H, W, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_stem_train_pack_input")
    return out


def stem_train(conv, bn, x):
    """ResNet's stem -- max-pool 3x3/s2/p1 of relu(bn(conv 7x7/s2/p3(x))) -- on the HIP training kernels (csrc/stem_train.hip) as a
    differentiable function of the stem's learnable tensors, the counterpart of ``basic_block_train``: ``x`` is a CUDA ``[n,3,H,W]`` tensor
    (fp32 or fp16, H and W even), the result ``[n,64,ceil(H/4),ceil(W/4)]`` fp32 that requires grad.  Frozen-statistics BatchNorm: the running
    statistics normalise and are never written.  The backward fills ``conv.weight.grad``, ``bn.weight.grad`` and ``bn.bias.grad``; the
    gradient for ``x`` is None."""
    tap = pack_image(x)
    geom, eps, learn, stats = _stem_operands(conv, bn, tap)
    return _StemTrainFn.apply(tap, geom, eps, tuple(stats), None, *learn)


_STEM_BN_MOMENTUM = ("the HIP batch-statistics stem kernels need a fixed momentum on the stem's BatchNorm (momentum=None, the cumulative average, "
                     "is not built)")


def _stem_bn_plan(bn, geom):
    """(training, momentum) for the vtd_stem_bn_train_* entries from the stem's BatchNorm, validated before the device is looked at."""
    if bn.momentum is None:
        raise ValueError(_STEM_BN_MOMENTUM)
    n, H, W = geom
    if bn.training and n * (H // 2) * (W // 2) < 2:
        raise ValueError(f"train-mode BatchNorm needs more than one value per channel, got a conv map of {n} x {H // 2} x {W // 2}")
    return (bool(bn.training), float(bn.momentum))


def stem_bn_train(conv, bn, x):
    """``stem_train`` on the vtd_stem_bn_train_* entries (csrc/stem_train.hip) with torch's module semantics, the counterpart of
    ``trunk_block_bn_train``: in ``bn.training`` mode the statistics of the batch normalise, ``bn.running_mean`` and ``bn.running_var`` are
    updated in place (the unbiased variance, the BatchNorm's own fixed momentum) and ``bn.num_batches_tracked`` advances; in ``eval()`` mode
    it gives the bits of ``stem_train(conv, bn, x)`` and writes no buffer.  Differentiable w.r.t. ``conv.weight``, ``bn.weight`` and
    ``bn.bias`` -- the full BatchNorm backward in train mode --; the gradient for ``x`` is None."""
    if isinstance(bn, nn.BatchNorm2d) and bn.momentum is None:      # what is built, before anything about the device
        raise ValueError(_STEM_BN_MOMENTUM)
    tap = pack_image(x)
    geom, eps, learn, stats = _stem_operands(conv, bn, tap)
    out = _StemTrainFn.apply(tap, geom, eps, tuple(stats), _stem_bn_plan(bn, geom), *learn)
    if bn.training:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
    return out


def forward_stem_padded(conv, bn, image_tap):
    """ResNet's stem on an image tap (nets.pack_image) with the HIP training kernels, no gradient: the pooled padded tap [n,hp+2,wp+2,64]
    fp16 with a zero ring, what forward_layer1_padded reads."""
    geom, eps, learn, stats = _stem_operands(conv, bn, image_tap)
    with torch.no_grad():
        return _stem_forward_raw(image_tap.detach(), geom, eps, [t.detach() for t in learn], stats)[0]


# ResNet-18's four residual stages, two BasicBlocks each (the first cin -> width at `stride`, the second width -> width at stride 1): `tap` names
# the stage's input, `operands` are the keywords of BasicBlock._train_operands that admit its geometries, `entry` is the entry family the stage
# runs on when it runs alone (forward_<stage>_padded, and the training node of layer4 alone)
_Stage = namedtuple("_Stage", "name cin width stride tap operands entry")
_STAGES = (_Stage("layer1", 64, 64, 1, "pool", {"general": True, "narrow": True}, "vtd_block64_train"),
           _Stage("layer2", 64, 128, 2, "C2", {"general": True}, "vtd_resblock_train"),
           _Stage("layer3", 128, 256, 2, "C3", {"general": True}, "vtd_resblock_train"),
           _Stage("layer4", 256, 512, 2, "C4", {}, "vtd_basicblock_train"))


def _stage_operands(stage, layer, tap, device=None):
    """One stage (a row of _STAGES) on a padded tap of its input: (the two blocks, their geometries, eps, their learnable tensors, their
    running statistics).  Only the tap's shape is read; `device` names the parameters' device when the tap is a shape-only stand-in."""
    name, cin, width, stride = stage.name, stage.cin, stage.width, stage.stride
    blocks = list(layer)
    if len(blocks) != 2 or not all(isinstance(b, BasicBlock) for b in blocks):
        raise RuntimeError(f"{name} training is built for ResNet-18's two BasicBlocks; Bottleneck training is not built")
    n, h, w = int(tap.shape[0]), int(tap.shape[1]) - 2, int(tap.shape[2]) - 2
    ops = [b._train_operands(tap.device if device is None else device, **stage.operands) for b in blocks]
    if [o[0] for o in ops] != [(cin, width, stride), (width, width, 1)] or tap.shape[3] != cin:
        built = f"{cin} -> {width} stride 1, twice" if stride == 1 else f"{cin} -> {width} stride {stride}, then {width} -> {width} stride 1"
        raise RuntimeError(f"{name} training is built for ResNet-18's {name} ({built})")
    if (stride == 2 and (h % 2 or w % 2)) or ops[0][1] != ops[1][1]:
        raise RuntimeError(f"{name} training needs " + (f"a {stage.tap} of even extents and " if stride == 2 else "") + "one BatchNorm eps")
    geoms = [(n, h, w, cin, width, stride), (n, h // stride, w // stride, width, width, 1)]
    return blocks, geoms, ops[0][1], [o[2] for o in ops], [tuple(o[3]) for o in ops]


def _forward_stage_padded(stage, layer, tap):
    _, geoms, eps, learn, stats = _stage_operands(stage, layer, tap)
    with torch.no_grad():
        mid, _ = _block_forward_raw(tap.detach(), geoms[0], eps, [t.detach() for t in learn[0]], stats[0], stage.entry)
        return _block_forward_raw(mid, geoms[1], eps, [t.detach() for t in learn[1]], stats[1], stage.entry)[0]


def forward_layer1_padded(layer1, pool_tap):
    """ResNet-18's layer1 on a padded tap of the pooled stem output with the HIP training kernels, no gradient: padded C2
    [n,h+2,w+2,64] fp16."""
    return _forward_stage_padded(_STAGES[0], layer1, pool_tap)


def forward_layer2_padded(layer2, c2_tap):
    """ResNet-18's layer2 on a padded C2 tap with the HIP training kernels, no gradient: padded C3 [n,h3+2,w3+2,128] fp16."""
    return _forward_stage_padded(_STAGES[1], layer2, c2_tap)


def forward_layer3_padded(layer3, c3_tap):
    """ResNet-18's layer3 on a padded C3 tap with the HIP training kernels, no gradient: padded C4 [n,h4+2,w4+2,256] fp16."""
    return _forward_stage_padded(_STAGES[2], layer3, c3_tap)


def forward_layer4_padded(layer4, c4_tap):
    """ResNet-18's layer4 on a padded C4 tap with the HIP training kernels, no gradient: padded C5 [n,h5+2,w5+2,512] fp16."""
    return _forward_stage_padded(_STAGES[3], layer4, c4_tap)


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


def _head_structs(params, buffers=None, grads=None):
    tensors, gtensors = {}, {}
    for b in range(2):
        for i, (field, _, _) in enumerate(_HEAD_LEARNABLE):
            tensors[(b, field)] = params[b * len(_HEAD_LEARNABLE) + i]
            if grads is not None:
                gtensors[(b, field)] = grads[b * len(_HEAD_LEARNABLE) + i]
        if buffers is not None:
            for i, (field, _, _) in enumerate(_HEAD_BUFFERS):
                tensors[(b, field)] = buffers[b * len(_HEAD_BUFFERS) + i]
    return _head_struct(tensors), (_head_struct(gtensors) if grads is not None else None)


def _head_forward_raw(feats, hw, training, momentum, eps, buffers, params):
    """vtd_dbhead_train_forward on padded features: (workspace, prob, thresh, stats)."""
    n, (H, W) = feats.shape[0], hw
    st, _ = _head_structs(params, buffers)
    dev = feats.device
    C, _native, lib, ws = _native_workspace("vtd_dbhead_train_workspace_bytes", (n, H, W, 0), dev)
    prob = torch.empty((n, 1, 4 * H, 4 * W), dtype=torch.float32, device=dev)
    thresh = torch.empty_like(prob)
    stats = torch.empty((4, 2, 64), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _native.check(lib.vtd_dbhead_train_forward(ptr(feats), n, H, W, C.byref(st), 1 if training else 0, float(momentum), float(eps), ptr(ws),
                                               ptr(prob), ptr(thresh), ptr(stats), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "vtd_dbhead_train_forward")
    return ws, prob, thresh, stats


def _head_backward_raw(feats, hw, training, ws, prob, thresh, params, grad_prob, grad_thresh, want_input):
    """vtd_dbhead_train_backward (+ _backward_input): (the 20 gradients, dfeats, dscale); dfeats is NHWC fp32 [n,H,W,256] times dscale[0]."""
    n, (H, W) = feats.shape[0], hw
    grads = [torch.empty_like(p) for p in params]
    st, gst = _head_structs(params, None, grads)
    C, _native, lib, scratch = _native_workspace("vtd_dbhead_train_workspace_bytes", (n, H, W, 2 if want_input else 1), feats.device)
    g = [None if t is None else t.to(torch.float32).contiguous() for t in (grad_prob, grad_thresh)]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(lib.vtd_dbhead_train_backward(ptr(feats), n, H, W, C.byref(st), 1 if training else 0, ptr(ws), ptr(prob),
                                                ptr(thresh), ptr(g[0]), ptr(g[1]), C.byref(gst), ptr(scratch), stream), "vtd_dbhead_train_backward")
    dfeats = dscale = None
    if want_input:
        dfeats = torch.empty((n, H, W, 256), dtype=torch.float32, device=feats.device)   # NHWC, scaled by dscale[0]
        dscale = torch.empty(2, dtype=torch.float32, device=feats.device)
        _native.check(lib.vtd_dbhead_train_backward_input(n, H, W, C.byref(st), ptr(scratch), ptr(dfeats), ptr(dscale), stream),
                      "vtd_dbhead_train_backward_input")
    return grads, dfeats, dscale


class _DBHeadTrainFn(torch.autograd.Function):
    """DBHead.forward on the HIP training kernels (csrc/dbhead_train.hip), differentiable w.r.t. the 20 learnable head tensors.  Inputs:
    padded features (include/vtd.h), `src`, (H, W), BatchNorm mode / momentum / eps, the four running-stat buffers per branch (updated in
    place in training mode), then the learnable tensors branch-major in _HEAD_LEARNABLE order.  `src` is None, or the [n,256,H,W] tensor the
    padded features were packed from: when it requires grad the backward also forms the gradient of the features (dgrad into P2,
    vtd_dbhead_train_backward_input) and hands it to `src` in NCHW."""

    @staticmethod
    def forward(ctx, feats, src, hw, training, momentum, eps, buffers, *params):
        ws, prob, thresh, stats = _head_forward_raw(feats, hw, training, momentum, eps, buffers, params)
        ctx.save_for_backward(feats, prob, thresh, *params)
        ctx.ws, ctx.hw, ctx.training = ws, tuple(hw), bool(training)
        ctx.src_dtype = None if src is None else src.dtype
        ctx.mark_non_differentiable(stats)
        return prob, thresh, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_prob, grad_thresh, _grad_stats):
        import ctypes as C
        from . import _native
        feats, prob, thresh, *params = ctx.saved_tensors
        n, (H, W) = feats.shape[0], ctx.hw
        want_input = ctx.src_dtype is not None and ctx.needs_input_grad[1]
        grads, dfeats, dscale = _head_backward_raw(feats, ctx.hw, ctx.training, ctx.ws, prob, thresh, params, grad_prob, grad_thresh, want_input)
        grad_src = None
        if want_input:
            lib = _native.require()
            ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            grad_src = torch.empty((n, 256, H, W), dtype=torch.float32, device=feats.device)
            _native.check(lib.vtd_dbhead_unpack_input_grad(ptr(dfeats), ptr(dscale), n, H, W, ptr(grad_src),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_dbhead_unpack_input_grad")
            grad_src = grad_src.to(ctx.src_dtype)
        return (None, grad_src, None, None, None, None, None, *grads)


# ---- BasicBlock training (csrc/resblock_train.hip).  geom = (n, h_in, w_in, cin, width, stride); learn = conv1.weight, bn1.weight, bn1.bias,
# conv2.*, bn2.*, then the downsample's three; stats = the running means and variances in the same order
def _block_struct(learn, stats=None, bottleneck=False):
    """vtd_basicblock_params over a BasicBlock's tensors, or with `bottleneck` vtd_bottleneck_params over a Bottleneck's (conv3 / bn3 third)."""
    import ctypes as C
    from . import _native
    st = _native.BottleneckParams() if bottleneck else _native.BasicBlockParams()
    pairs = ("conv1_w bn1_w bn1_b", "conv2_w bn2_w bn2_b") + (("conv3_w bn3_w bn3_b",) if bottleneck else ()) + ("ds_w ds_bn_w ds_bn_b",)
    for i, pre in enumerate(pairs[:len(learn) // 3]):
        for j, field in enumerate(pre.split()):
            setattr(st, field, C.c_void_p(learn[3 * i + j].data_ptr()))
        if stats is not None:
            bn = pre.split()[1][:-2]
            setattr(st, bn + "_mean", C.c_void_p(stats[2 * i].data_ptr()))
            setattr(st, bn + "_var", C.c_void_p(stats[2 * i + 1].data_ptr()))
    return st


_BASICBLOCK = "vtd_basicblock_train"   # the entry family of layer4's two geometries (no strided dgrad)
_RESBLOCK = "vtd_resblock_train"       # the entry family of the six geometries of layer2, layer3 and layer4
_BLOCK64 = "vtd_block64_train"         # the entry family of layer1's 64 -> 64 block
_RESBLOCK_BN = "vtd_resblock_bn_train"   # layer4's two geometries with batch-statistics BatchNorm (csrc/resblock_bn_train.hip)
_BLOCK_BN = "vtd_block_bn_train"         # layer3's and layer4's four with batch-statistics BatchNorm, and the strided dx (the same file)
_TRUNK_BN = "vtd_trunk_bn_train"         # layer2's two and layer1's one as well, seven in all (the same file); the stem's batch-statistics
                                         # entries, vtd_stem_bn_train_*, are csrc/stem_train.hip's
_BOTTLENECK = "vtd_bottleneck_train"     # ResNet-50's last stage: the two Bottleneck geometries of width 512 (csrc/bottleneck_train.hip); the
                                         # block's output has 4 width channels and its struct a third convolution + BatchNorm pair
_BOTTLENECK256 = "vtd_bottleneck256_train"   # ResNet-50's res4: the two Bottleneck geometries of width 256, the same file and struct
_BOTTLENECK128 = "vtd_bottleneck128_train"   # ResNet-50's res3: the two Bottleneck geometries of width 128, the same file and struct
_BOTTLENECK64 = "vtd_bottleneck64_train"     # ResNet-50's res2: the two Bottleneck geometries of width 64 (both stride 1), the same file and struct
_BOTTLENECK_FAMILIES = (_BOTTLENECK, _BOTTLENECK256, _BOTTLENECK128, _BOTTLENECK64)
_BOTTLENECK_BN = "vtd_bottleneck_bn_train"   # res5's and res4's four Bottleneck geometries with batch-statistics BatchNorm
                                             # (csrc/bottleneck_bn_train.hip): the Bottleneck struct, the 4 width output, statistics [4,2,4 width]
_BOTTLENECK_STRUCT = _BOTTLENECK_FAMILIES + (_BOTTLENECK_BN,)   # the families on vtd_bottleneck_params
_BN_FAMILIES = (_BLOCK_BN, _TRUNK_BN, _BOTTLENECK_BN)   # the batch-statistics families a caller names itself; any other entry means
                                                        # vtd_resblock_bn_train

# ResNet-50's four residual stages, lowest first, as _STAGES is ResNet-18's: `slot` is the stage's place in the backbone, `blocks` the count
# of its Bottlenecks (the first cin -> width -> 4 width at `stride`, the others 4 width -> width -> 4 width at stride 1), `tap` names the
# stage's input, `entry` is its entry family with frozen-statistics BatchNorm, `geometries` and `family_built` are what that family runs
# and its refusal, `built` is the stage's own refusal
_ResStage = namedtuple("_ResStage", "name slot blocks cin width stride tap entry geometries family_built built")
_RES_STAGES = (_ResStage("res2", 4, 3, 64, 64, 1, "pool", _BOTTLENECK64, _BOTTLENECK64_GEOMETRIES, _BOTTLENECK64_BUILT, _RES2_BUILT),
               _ResStage("res3", 5, 4, 256, 128, 2, "C2", _BOTTLENECK128, _BOTTLENECK128_GEOMETRIES, _BOTTLENECK128_BUILT, _RES3_BUILT),
               _ResStage("res4", 6, 6, 512, 256, 2, "C3", _BOTTLENECK256, _BOTTLENECK256_GEOMETRIES, _BOTTLENECK256_BUILT, _RES4_BUILT),
               _ResStage("res5", 7, 3, 1024, 512, 2, "C4", _BOTTLENECK, _BOTTLENECK_GEOMETRIES, _BOTTLENECK_BUILT, _RES5_BUILT))


def _listed(names):
    """The names as a phrase: 'a', 'a and b', 'a, b and c'."""
    return " and ".join(filter(None, (", ".join(names[:-1]), names[-1])))


def _block_entry(geom):
    """The entry family of a block of basic_block_train's seven, by its width."""
    return _BLOCK64 if geom[4] == 64 else _RESBLOCK


def _block_forward_raw(tap, geom, eps, learn, stats, entry=_BASICBLOCK, bn=None):
    """vtd_basicblock_train_forward (or `entry`'s) on a padded tap: (padded y [n,h+2,w+2,width] fp16, workspace).  With `bn` = (training,
    momentum) it is vtd_resblock_bn_train_forward (vtd_block_bn_train_forward when `entry` names that family), which takes the two after the
    parameters, and the result has a third member: the batch
    statistics [3,2,width] fp32 -- mu and the biased variance of bn1, bn2 and the downsample's BatchNorm; rows the call does not write are
    NaN.  In training mode the running statistics in `stats` are then updated in place."""
    entry = entry if bn is None or entry in _BN_FAMILIES else _RESBLOCK_BN
    C, _native, lib, ws = _native_workspace(entry + "_workspace_bytes", (*geom, 0), tap.device)
    n, hin, win, cin, width, stride = geom
    y = torch.empty((n, hin // stride + 2, win // stride + 2, 4 * width if entry in _BOTTLENECK_STRUCT else width), dtype=torch.float16, device=tap.device)
    mode = () if bn is None else (1 if bn[0] else 0, float(bn[1]))
    # vtd_bottleneck_bn_train's statistics are [4,2,4 width]: bn1, bn2, bn3, the downsample's; the first two rows use the first `width` columns
    bshape = (4, 2, 4 * width) if entry == _BOTTLENECK_BN else (3, 2, width)
    bstats = () if bn is None else (torch.full(bshape, float("nan"), dtype=torch.float32, device=tap.device),)
    st = _block_struct(learn, stats, entry in _BOTTLENECK_STRUCT)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _native.check(getattr(lib, entry + "_forward")(ptr(tap), *geom, C.byref(st), *mode, eps, ptr(ws), ptr(y), *map(ptr, bstats),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), entry + "_forward")
    return (y, ws, *bstats)


def _block_backward_raw(tap, geom, eps, learn, stats, ws, y, dy, dscale, want_dx, entry=_BASICBLOCK, bn=None):
    """vtd_basicblock_train_backward (or `entry`'s) on dy as NHWC fp32 times dscale[0]: (the gradients in the order of `learn`, dx, dxscale);
    dx is NHWC fp32 [n,h_in,w_in,cin] times dxscale[0], or None.  With `bn` = (training, momentum) it is vtd_resblock_bn_train_backward,
    which takes the mode after the parameters and forms dx for the stride-1 block only, or when `entry` names that family
    vtd_block_bn_train_backward, which forms dx for either stride."""
    entry = entry if bn is None or entry in _BN_FAMILIES else _RESBLOCK_BN
    grads = [torch.empty_like(p) for p in learn]
    C, _native, lib, scratch = _native_workspace(entry + "_workspace_bytes", (*geom, 1), tap.device)
    n, hin, win, cin, width, stride = geom
    st, gst = _block_struct(learn, stats, entry in _BOTTLENECK_STRUCT), _block_struct(grads, None, entry in _BOTTLENECK_STRUCT)
    dx = torch.empty((n, hin, win, cin), dtype=torch.float32, device=tap.device) if want_dx else None
    dxs = torch.empty(2, dtype=torch.float32, device=tap.device) if want_dx else None
    mode = () if bn is None else (1 if bn[0] else 0,)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _native.check(getattr(lib, entry + "_backward")(ptr(tap), *geom, C.byref(st), *mode, eps, ptr(ws), ptr(y), ptr(dy), ptr(dscale), C.byref(gst),
                                                    ptr(scratch), ptr(dx), ptr(dxs), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  entry + "_backward")
    return grads, dx, dxs


def _combine_scaled(a, ascale, b, bscale):
    """vtd_resblock_train_combine: a <- a + b with both brought to the smaller of their two power-of-two scales; (a, that scale [2])."""
    import ctypes as C
    from . import _native
    lib = _native.require()
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _native.check(lib.vtd_resblock_train_combine(ptr(a), ptr(ascale), ptr(b), ptr(bscale), a.numel(), ptr(out),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_resblock_train_combine")
    return a, out


class _BlockTrainFn(torch.autograd.Function):
    """One BasicBlock on the HIP training kernels: padded tap in, [n,width,h,w] fp32 out.  `entry` is the entry family: vtd_basicblock_train
    (layer4's two geometries; `src` for the stride-1 block only), vtd_resblock_train or vtd_block64_train (the seven geometries, `src` for
    either stride), or with `bn` = (training, momentum) vtd_resblock_bn_train (csrc/resblock_bn_train.hip): `training` selects batch
    statistics (the running statistics in `stats` are then updated in place) or the frozen path.  `src` is None or the NCHW tensor the tap
    was packed from: when it requires grad it receives the input gradient in its own dtype."""

    @staticmethod
    def forward(ctx, tap, src, geom, eps, stats, entry, bn, *learn):
        y, ws = _block_forward_raw(tap, geom, eps, learn, stats, entry, bn)[:2]
        ctx.save_for_backward(tap, y, *stats, *learn)
        ctx.ws, ctx.geom, ctx.eps, ctx.nstats, ctx.entry, ctx.bn = ws, geom, eps, len(stats), entry, bn
        ctx.src_dtype = None if src is None else src.dtype
        return y[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        tap, y, *rest = ctx.saved_tensors
        stats, learn = rest[:ctx.nstats], rest[ctx.nstats:]
        dy = grad_out.to(torch.float32).permute(0, 2, 3, 1).contiguous()
        dscale = torch.ones(2, dtype=torch.float32, device=dy.device)
        want_dx = ctx.src_dtype is not None and ctx.needs_input_grad[1]
        grads, dx, dxs = _block_backward_raw(tap, ctx.geom, ctx.eps, learn, stats, ctx.ws, y, dy, dscale, want_dx, ctx.entry, ctx.bn)
        gsrc = _fpn_unpack_tap_grad(dx, dxs).to(ctx.src_dtype) if want_dx else None
        return (None, gsrc, None, None, None, None, None, *grads)


# ---- FPN training (csrc/fpn_train.hip).  geom = (n, h5, w5, c5 channels); taps = padded taps C2..C5; params = the ten live tensors:
# inner_blocks[0..3].weight, inner_blocks[0..3].bias, layer_blocks[3].weight, layer_blocks[3].bias
def _fpn_struct(tensors):
    import ctypes as C
    from . import _native
    st = _native.FpnParams()
    for i in range(4):
        st.inner_w[i] = C.c_void_p(tensors[i].data_ptr())
        st.inner_b[i] = C.c_void_p(tensors[4 + i].data_ptr())
    st.layer_w = C.c_void_p(tensors[8].data_ptr())
    st.layer_b = C.c_void_p(tensors[9].data_ptr())
    return st


def _fpn_taps(taps):
    import ctypes as C
    from . import _native
    return _native.FpnTaps(*(C.c_void_p(t.data_ptr()) for t in taps))


def _fpn_forward_raw(taps, geom, params):
    """vtd_fpn_train_forward: (padded P2 [n,8 h5 + 2,8 w5 + 2,256] fp16, workspace)."""
    n, h5, w5, c5 = geom
    dev = taps[0].device
    C, _native, lib, ws = _native_workspace("vtd_fpn_train_workspace_bytes", (n, h5, w5, c5, 0), dev)
    p2 = torch.empty((n, 8 * h5 + 2, 8 * w5 + 2, 256), dtype=torch.float16, device=dev)
    st, tp = _fpn_struct(params), _fpn_taps(taps)
    _native.check(lib.vtd_fpn_train_forward(C.byref(tp), n, h5, w5, c5, C.byref(st), C.c_void_p(ws.data_ptr()), C.c_void_p(p2.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_fpn_train_forward")
    return p2, ws


def _fpn_backward_raw(taps, geom, params, ws, dp2, dscale, input_mask=0):
    """vtd_fpn_train_backward on dP2 as NHWC fp32 times dscale[0]: the ten gradients, in the order of `params`.  With `input_mask` (bit lv
    asks for C(2 + lv)) also vtd_fpn_train_backward_input: (the ten gradients, [dC2..dC5] with None for levels not asked for, their scales
    [4,2]); each dC(k) is NHWC fp32 [n,h,w,C] times its scales[lv, 0]."""
    n, h5, w5, c5 = geom
    grads = [torch.empty_like(p) for p in params]
    query = ("vtd_fpn_train_input_workspace_bytes", (n, h5, w5, c5)) if input_mask else ("vtd_fpn_train_workspace_bytes", (n, h5, w5, c5, 1))
    C, _native, lib, scratch = _native_workspace(*query, dp2.device)
    st, gst, tp = _fpn_struct(params), _fpn_struct(grads), _fpn_taps(taps)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(lib.vtd_fpn_train_backward(C.byref(tp), n, h5, w5, c5, C.byref(st), ptr(ws), ptr(dp2), ptr(dscale), C.byref(gst), ptr(scratch),
                                             stream), "vtd_fpn_train_backward")
    if not input_mask:
        return grads
    dtaps = [torch.empty((n, h5 << (3 - lv), w5 << (3 - lv), c5 >> (3 - lv)), dtype=torch.float32, device=dp2.device) if (input_mask >> lv) & 1 else None
             for lv in range(4)]
    scales = torch.zeros((4, 2), dtype=torch.float32, device=dp2.device)
    out = _native.FpnTaps(*(None if t is None else ptr(t) for t in dtaps))
    _native.check(lib.vtd_fpn_train_backward_input(n, h5, w5, c5, C.byref(st), ptr(scratch), int(input_mask), C.byref(out), ptr(scales), stream),
                  "vtd_fpn_train_backward_input")
    return grads, dtaps, scales


def _fpn_unpack_tap_grad(dtap, scale):
    """vtd_fpn_train_unpack_tap_grad: NHWC fp32 [n,h,w,C] times scale[0] -> [n,C,h,w] fp32, the scale undone."""
    import ctypes as C
    from . import _native
    lib = _native.require()
    n, h, w, ch = dtap.shape
    out = torch.empty((n, ch, h, w), dtype=torch.float32, device=dtap.device)
    _native.check(lib.vtd_fpn_train_unpack_tap_grad(C.c_void_p(dtap.data_ptr()), C.c_void_p(scale.data_ptr()), n, ch, h, w, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_fpn_train_unpack_tap_grad")
    return out


class _FPNTrainFn(torch.autograd.Function):
    """The FPN alone on the HIP training kernels: padded taps in, P2 as [n,256,H,W] fp32 out, differentiable w.r.t. the ten live tensors.
    `s2..s5` are None, or the [n,C,H,W] tensors the padded taps were packed from: those that require grad receive their gradient
    (vtd_fpn_train_backward_input, only the levels that need one) in their own dtype."""

    @staticmethod
    def forward(ctx, taps, geom, s2, s3, s4, s5, *params):
        import ctypes as C
        from . import _native
        lib = _native.require()
        p2p, ws = _fpn_forward_raw(taps, geom, params)
        n, h5, w5, _ = geom
        out = torch.empty((n, 256, 8 * h5, 8 * w5), dtype=torch.float32, device=p2p.device)
        _native.check(lib.vtd_fpn_train_unpack_p2(C.c_void_p(p2p.data_ptr()), n, 8 * h5, 8 * w5, C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_fpn_train_unpack_p2")
        ctx.save_for_backward(*params)
        ctx.taps, ctx.geom, ctx.ws = taps, geom, ws
        ctx.src_dtypes = tuple(None if t is None else t.dtype for t in (s2, s3, s4, s5))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        import ctypes as C
        from . import _native
        lib = _native.require()
        n, h5, w5, _ = ctx.geom
        g = grad_out.to(torch.float32).contiguous()
        dp2 = torch.empty((n, 8 * h5, 8 * w5, 256), dtype=torch.float32, device=g.device)
        _native.check(lib.vtd_fpn_train_pack_grad(C.c_void_p(g.data_ptr()), n, 8 * h5, 8 * w5, C.c_void_p(dp2.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vtd_fpn_train_pack_grad")
        dscale = torch.ones(2, dtype=torch.float32, device=g.device)
        mask = sum(1 << lv for lv in range(4) if ctx.src_dtypes[lv] is not None and ctx.needs_input_grad[2 + lv])
        if not mask:
            return (None, None, None, None, None, None, *_fpn_backward_raw(ctx.taps, ctx.geom, ctx.saved_tensors, ctx.ws, dp2, dscale))
        grads, dtaps, scales = _fpn_backward_raw(ctx.taps, ctx.geom, ctx.saved_tensors, ctx.ws, dp2, dscale, mask)
        dsrc = [None if t is None else _fpn_unpack_tap_grad(t, scales[lv]).to(ctx.src_dtypes[lv]) for lv, t in enumerate(dtaps)]
        return (None, None, *dsrc, *grads)


# What one run of the trunk node is, built by FeaturePyramidNetwork.forward_padded.  _TrunkPlan: `taps` the padded taps the node reads, `geom`
# the FPN's geometry, `head` the head's (BatchNorm mode, momentum, eps, running-stat buffers), `stem` None or the stem's (geometry, eps,
# running statistics) with (training, momentum) as a fourth entry for the vtd_stem_bn_train_* entries, `blocks` a _BlockPlan for each
# BasicBlock from the lowest up (none: the FPN and the head alone) with `beps` their eps,
# `bn` None or (training, momentum) for blocks on the batch-statistics entries.  _BlockPlan: the block's geometry, its running statistics,
# its entry family and the count of its learnable tensors (9 with a downsample, 6 without; a Bottleneck's 12 and 9).  `per`: the blocks of
# each stage of the plan, 2 for ResNet-18's BasicBlock stages and 3 for ResNet-50's res5 alone; an int means "every stage", a tuple gives
# every stage its own count from the lowest up (_RES_STAGES' block counts).  A stage's last block is a C(k)
_TrunkPlan = namedtuple("_TrunkPlan", "taps geom head stem blocks beps bn per", defaults=(2,))
_BlockPlan = namedtuple("_BlockPlan", "geom stats entry nlearn")


class _TrunkFPNHeadTrainFn(torch.autograd.Function):
    """[stem ->] [layer1 ->] [layer2 ->] [layer3 ->] [layer4 ->] FPN -> DB head as one node on padded taps, at whatever depth `plan` says.
    Inputs: the plan, then the learnable tensors: the stem's 3 if it runs, those of the blocks from the lowest up, the FPN's 10, the head's 20.

    Forward: the stem's launch on the image tap if there is one, then the blocks in order, each on the tap the one before wrote; the last
    tap of plan.taps is the lowest block's input otherwise.  C2 .. C5 are the taps given and the output of every stage's last block, the
    stages being plan.per blocks each (ResNet-50's Bottleneck stages: a tuple of their counts from the lowest up).

    Backward: head -> FPN -> the blocks from the top down, every gradient handed on as the kernels leave it (NHWC fp32 with its power-of-two
    scale), never through fp16 or an NCHW copy.  The FPN's backward forms dC(k) for the levels the node computes itself (the top
    stages of the plan); dC5 goes into the last block.  Every block but the lowest forms its input gradient (a stage's first block: the strided
    dgrad); where a stage's input is an FPN level too, the first block's dx and the FPN's dC(k) of that level are added at one power-of-two
    scale (vtd_resblock_train_combine) before they go into the stage below.  The lowest block forms a dx only when the stem runs, and that dx
    is the stem's dpool.  The parameter gradients of a block do not depend on whether its dx is formed, so a node gives the bits of the node
    one stage shallower on the taps that stage produces."""

    @staticmethod
    def _stages(plan):
        """(the index of every stage's first block, of its last block), from the lowest stage up."""
        sizes = (plan.per,) * (len(plan.blocks) // plan.per) if isinstance(plan.per, int) else tuple(plan.per)
        firsts = [sum(sizes[:k]) for k in range(len(sizes))]
        return firsts, [f + s - 1 for f, s in zip(firsts, sizes)]

    @staticmethod
    def _split(plan, params):
        """(the stem's tensors, the blocks', the FPN's, the head's) out of the node's flat parameter list."""
        cuts = [3 if plan.stem is not None else 0]
        for b in plan.blocks:
            cuts.append(cuts[-1] + b.nlearn)
        blocks = [params[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        return params[:cuts[0]], blocks, params[cuts[-1]:cuts[-1] + 10], params[cuts[-1] + 10:]

    @staticmethod
    def forward(ctx, plan, *params):
        slearn, blearn, fpn_params, head_params = _TrunkFPNHeadTrainFn._split(plan, params)
        n, h5, w5, _ = plan.geom
        hw = (8 * h5, 8 * w5)
        training, momentum, eps, hbuffers = plan.head
        x, stem_saved = plan.taps[-1], ()
        if plan.stem is not None:
            sgeom, seps, sstats, *sbn = plan.stem      # sbn: nothing, or [(training, momentum)] for the batch-statistics entries
            x, idx, ctx.sws = _stem_forward_raw(plan.taps[0], sgeom, seps, slearn, sstats, *sbn)
            stem_saved = (x, idx)
        acts, bws = [], []
        lasts = _TrunkFPNHeadTrainFn._stages(plan)[1]
        for b, learn in zip(plan.blocks, blearn):      # acts: each block's output; that of every stage's last block is a C(k)
            x, ws = _block_forward_raw(x, b.geom, plan.beps, learn, b.stats, b.entry, plan.bn)[:2]
            acts.append(x)
            bws.append(ws)
        ftaps = (*plan.taps, *(acts[j] for j in lasts))[-4:]      # C2 .. C5: the last four (an image or pooled tap in front falls out)
        p2p, fws = _fpn_forward_raw(ftaps, plan.geom, fpn_params)
        hws, prob, thresh, stats = _head_forward_raw(p2p, hw, training, momentum, eps, hbuffers, head_params)
        ctx.save_for_backward(p2p, prob, thresh, *stem_saved, *acts, *params)
        ctx.plan, ctx.hw, ctx.fws, ctx.hws, ctx.bws = plan, hw, fws, hws, tuple(bws)
        ctx.mark_non_differentiable(stats)
        return prob, thresh, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_prob, grad_thresh, _grad_stats):
        plan, nb = ctx.plan, len(ctx.plan.blocks)
        p2p, prob, thresh, *rest = ctx.saved_tensors
        nstem = 2 if plan.stem is not None else 0
        stem_saved, acts, params = rest[:nstem], rest[nstem:nstem + nb], rest[nstem + nb:]
        slearn, blearn, fpn_params, head_params = _TrunkFPNHeadTrainFn._split(plan, params)
        hgrads, dp2, dscale = _head_backward_raw(p2p, ctx.hw, bool(plan.head[0]), ctx.hws, prob, thresh, head_params, grad_prob, grad_thresh, True)
        firsts, lasts = _TrunkFPNHeadTrainFn._stages(plan)
        ftaps = (*plan.taps, *(acts[j] for j in lasts))[-4:]
        stages = len(firsts)
        fout = _fpn_backward_raw(ftaps, plan.geom, fpn_params, ctx.fws, dp2, dscale, sum(8 >> j for j in range(stages)))      # dC5 down
        if not plan.blocks:
            return (None, *fout, *hgrads)
        fgrads, dtaps, scales = fout
        ins = ((stem_saved[0] if plan.stem is not None else plan.taps[-1]), *acts[:-1])
        bgrads, d, ds = [None] * nb, dtaps[3], scales[3]
        for i in reversed(range(nb)):
            b, want_dx = plan.blocks[i], i > 0 or plan.stem is not None
            bgrads[i], d, ds = _block_backward_raw(ins[i], b.geom, plan.beps, blearn[i], b.stats, ctx.bws[i], acts[i], d, ds, want_dx, b.entry, plan.bn)
            if want_dx and i in firsts:
                level = 3 - stages + firsts.index(i)      # the FPN level of this block's stage's input: C(2 + level), none below C2
                if level >= 0:
                    d, ds = _combine_scaled(d, ds, dtaps[level], scales[level])      # the stage's share of dC(k) + the FPN's
        sgrads = ()
        if plan.stem is not None:      # layer1.0's input gradient is the stem's dpool
            sgeom, seps, sstats, *sbn = plan.stem
            sgrads = _stem_backward_raw(plan.taps[0], sgeom, seps, slearn, sstats, ctx.sws, *stem_saved, d, ds, *sbn)
        return (None, *sgrads, *(g for gs in bgrads for g in gs), *fgrads, *hgrads)


def pack_tap(feature):
    """[n,C,H,W] float32 / float16 CUDA tensor (C a multiple of 64) -> a padded tap (ring-padded NHWC fp16 [n,H+2,W+2,C]) on the device."""
    import ctypes as C
    from . import _native
    lib = _native.require()
    x = feature.detach()
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = x.contiguous()
    n, ch, H, W = x.shape
    out = torch.empty((n, H + 2, W + 2, ch), dtype=torch.float16, device=x.device)
    _native.check(lib.vtd_fpn_train_pack_tap(C.c_void_p(x.data_ptr()), 0 if x.dtype == torch.float32 else 1, n, ch, H, W,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "vtd_fpn_train_pack_tap")
    return out


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

    def _train_operands(self, device):
        """(the four BatchNorms, the 20 learnable tensors, the 8 running-stat buffers) as the kernels take them, validated."""
        if self.in_channels != 256:
            raise ValueError("the HIP DB-head kernels are specialised for 256 input channels")
        bns = [seq[i] for seq in self._branches() for i in (1, 4)]
        if any(bn.momentum is None or bn.momentum != bns[0].momentum or bn.eps != bns[0].eps or not bn.track_running_stats for bn in bns):
            raise ValueError("the HIP DB-head kernels need one fixed momentum and eps on all four BatchNorms, with running stats tracked")
        params, buffers = [], []
        for seq in self._branches():
            params += [getattr(seq[i], a) for _, i, a in _HEAD_LEARNABLE]
            buffers += [getattr(seq[i], a) for _, i, a in _HEAD_BUFFERS]
        for t in params + buffers:
            if not t.is_cuda or t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("DBHead parameters and buffers must be contiguous float32 CUDA tensors on the features' device "
                                 "(call .cuda() on the model)")
        return bns, params, buffers

    def _forward_padded(self, feats, H, W, src):
        if self.in_channels != 256:
            raise ValueError("the HIP DB-head kernels are specialised for 256 input channels")
        H, W = int(H), int(W)
        # the kernels trust the buffer's extent: a mismatch here would be a device-side out-of-bounds read
        if (not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float16 or not feats.is_contiguous() or feats.dim() != 4
                or H < 1 or W < 1 or feats.shape[0] < 1 or tuple(feats.shape[1:]) != (H + 2, W + 2, 256)):
            raise ValueError(f"padded features must be a contiguous float16 CUDA tensor [n,{H + 2},{W + 2},256] (H={H}, W={W}), got "
                             f"{tuple(feats.shape) if torch.is_tensor(feats) else type(feats).__name__}")
        bns, params, buffers = self._train_operands(feats.device)
        prob, thresh, _ = _DBHeadTrainFn.apply(feats, src, (int(H), int(W)), self.training, bns[0].momentum, bns[0].eps, tuple(buffers), *params)
        self._batches_seen(bns)
        return {"probability": prob, "threshold": thresh}

    def _batches_seen(self, bns):
        """After a forward on the training kernels, which update the running statistics themselves: num_batches_tracked + 1 on the four
        BatchNorms in training mode, as torch's modules count."""
        if self.training:
            with torch.no_grad():
                for bn in bns:
                    bn.num_batches_tracked.add_(1)


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


# the modes that train residual stages, each one stage further down than the one before (ResNet-18 only)
_STAGE_MODES = ("head+fpn+layer4", "head+fpn+layer4+layer3", "head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3+layer2+layer1")
# the whole detector: the four stages and the stem (ResNet-18 only); nothing is frozen and the train-mode forward needs no trunk engine
_BACKBONE_MODE = "head+fpn+backbone"
# ResNet-50's last stage, res5 (backbone.7: three Bottlenecks), with the FPN and the head; frozen-statistics BatchNorm (ResNet-50 only)
_RES5_MODE = "head+fpn+res5"
# one stage further down: res4 (backbone.6: six Bottlenecks of width 256) too, the upper two stages of ResNet-50 with the FPN and the head
_RES4_MODE = "head+fpn+res5+res4"
# and one more: res3 (backbone.5: four Bottlenecks of width 128); the trunk engine then stops at C2
_RES3_MODE = "head+fpn+res5+res4+res3"
# and the last residual stage: res2 (backbone.4: three Bottlenecks of width 64); the trunk engine then runs the stem alone (forward_pool)
_RES2_MODE = "head+fpn+res5+res4+res3+res2"
_RES_MODES = (_RES5_MODE, _RES4_MODE, _RES3_MODE, _RES2_MODE)
# the whole ResNet-50 detector: the four stages and the stem; nothing is frozen and the train-mode forward needs no trunk engine.  ResNet-18's
# name for the same, "head+fpn+backbone", stays refused on resnet50
_RES_WHOLE_MODE = "head+fpn+res5+res4+res3+res2+stem"
# what _RES_MODES and _RES_WHOLE_MODE name, and how ResNet-18's mode of the same depth (_STAGE_MODES, _BACKBONE_MODE) says it
_RES_MODE_NAMES = (("last stage (three Bottlenecks)", "the last stage trains"), ("upper two stages (nine Bottlenecks)", "the upper two stages train"),
                   ("upper three stages (thirteen Bottlenecks)", "the upper three stages train"),
                   ("four stages (sixteen Bottlenecks)", "the four stages train"), ("four stages and stem", "the whole detector trains"))


class DBNet(_EngineOwner, nn.Module):
    """DBNet detector network (text_detector.py:12-29), compute on the HIP engine.

    ``forward(x)`` accepts what the reference's ``TextDetector`` feeds it -- a
    normalised float NCHW tensor ``[B,3,640,640]`` -- or a ``DeviceFrames`` batch
    produced by the fused preprocess kernel, and returns
    ``{'probability': [B,1,640,640] f32 cuda tensor, 'threshold': same or None}``.
    """

    def __init__(self, backbone="resnet50", pretrained=False, compute_threshold=False, trainable=None, trunk_bn="frozen"):
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
        self.trunk_bn = "frozen"
        self.set_trainable(trainable, trunk_bn)

    def set_trainable(self, trainable, trunk_bn=None):
        """`trunk_bn` ("frozen", the default, "batch", "trained", or a tuple of stage names; None keeps the current value) is the mode of the
        trained trunk stages' BatchNorms.  "trained" (resnet18 with trainable="head+fpn+layer4", "head+fpn+layer4+layer3",
        "head+fpn+layer4+layer3+layer2" or "head+fpn+layer4+layer3+layer2+layer1"; anything else raises ValueError and leaves the network as it
        was): every residual stage the mode trains runs its BatchNorms in train mode.  On the first two modes it behaves as the tuples
        ("layer4",) and ("layer3", "layer4") do.  On the third the trunk engine gives C2 as with "frozen", then layer2, layer3 and layer4 run on
        the vtd_trunk_bn_train_* entries -- backbone.5 .. backbone.7's fifteen BatchNorms normalise with the statistics of the batch, and their
        30 running buffers and 15 counters move every step; a following eval() forward rebuilds the inference engine on the new statistics.
        On the fourth the trunk engine gives the pooled stem output as with "frozen", then layer1 .. layer4 run on the same entries:
        backbone.4 .. backbone.7's nineteen BatchNorms (layer1's blocks have no downsample), 38 running buffers and 19 counters.  The stem keeps
        frozen statistics under "trained": "head+fpn+backbone" with "trained" is refused.
        "bottleneck" (resnet50 with trainable="head+fpn+res5" or "head+fpn+res5+res4" only; on resnet18, with the other three ResNet-50 modes
        and with None / "head" / "head+fpn" it raises ValueError and leaves the network as it was): the trained Bottleneck stages run on the
        vtd_bottleneck_bn_train_* entries (csrc/bottleneck_bn_train.hip) in train mode -- backbone.7's ten BatchNorms normalise with the
        statistics of the batch and their 20 running buffers and 10 counters move every step; with res4 backbone.6's too, 29 BatchNorms, 58
        buffers and 29 counters.  The frozen part of the trunk comes from the trunk engine as with "frozen"; a following eval() forward
        rebuilds the inference engine on the moved statistics.  res3, res2 and the stem under batch statistics are not built: the follow-up.
        "backbone" (resnet18 with trainable="head+fpn+backbone" only; anything else raises ValueError and leaves the network as it was): the
        whole-backbone node with the stem on the vtd_stem_bn_train_* entries and layer1 .. layer4 on vtd_trunk_bn_train_* -- all twenty
        BatchNorms of the trunk normalise with the statistics of the batch, as the reference's model.train() step does, and their 40 running
        buffers and 20 counters move every step.
        A tuple names exactly the residual stages the mode trains, else ValueError: ("layer4",) goes with
        trainable="head+fpn+layer4" and is equivalent to "batch"; ("layer3", "layer4") goes with trainable="head+fpn+layer4+layer3" on resnet18:
        the trunk engine gives C2 and C3 as with "frozen", then layer3 and layer4 run on the vtd_block_bn_train_* entries -- backbone.6's and
        backbone.7's ten BatchNorms normalise with the statistics of the batch, and their 20 running buffers and 10 counters move every step.
        "frozen": as described below, the running statistics normalise and are never written.  "batch" (accepted only with
        trainable="head+fpn+layer4" on resnet18; every other combination raises ValueError): a forward in train mode runs the frozen trunk
        engine for C2..C4 exactly as with "frozen", then layer4 on csrc/resblock_bn_train.hip -- backbone.7's five BatchNorms normalise with
        the statistics of the batch, as the reference's model.train() step does, and their running statistics and num_batches_tracked move
        every step; a following eval() forward rebuilds the inference engine on the new statistics.  The state dict is the same in
        either mode.

        "head+fpn+res5" (ResNet-50 only; on resnet18 it raises ValueError that names "head+fpn+layer4"): fine-tune ResNet-50's last stage with the
        FPN and the head -- backbone.0 .. backbone.6 stop requiring grad; backbone.7 (three Bottlenecks, 30 tensors), fpn and head train.  A
        forward in train mode takes C2..C4 from the trunk engine (keyed on the frozen backbone tensors only; its own C5 is ignored), then runs
        res5 (csrc/bottleneck_train.hip), the FPN and the head on the HIP training kernels as one autograd node.  res5's BatchNorms normalise
        with their running statistics, which are never written: trunk_bn must be "frozen".

        "head+fpn+res5+res4" (ResNet-50 only; on resnet18 it raises ValueError that names "head+fpn+layer4+layer3"): the usual fine-tuning
        recipe of a detection trunk on the reference's own backbone -- backbone.0 .. backbone.5 stop requiring grad; backbone.6 (six
        Bottlenecks of width 256, 57 tensors), backbone.7 (30), fpn (10) and head (20) train: 117 tensors.  A forward in train mode takes C2
        and C3 from the trunk engine (keyed on the frozen backbone tensors only; its own C4 and C5 are ignored), then runs res4, res5, the
        FPN and the head on the HIP training kernels as one autograd node.  Frozen statistics only: trunk_bn must be "frozen".

        "head+fpn+res5+res4+res3+res2" (ResNet-50 only; on resnet18 it raises ValueError that names
        "head+fpn+layer4+layer3+layer2+layer1"): every residual stage -- only the stem (backbone.0, backbone.1) stops requiring grad;
        backbone.4 (three Bottlenecks of width 64, 30 tensors) and the 156 above train: 186 tensors.  A forward in train mode takes the
        pooled stem output from the trunk engine's forward_pool (keyed on the frozen stem tensors only; the stem alone runs), then runs res2
        .. res5, the FPN and the head on the HIP training kernels as one autograd node.  Frozen statistics only: trunk_bn must be "frozen".

        "head+fpn+res5+res4+res3+res2+stem" (ResNet-50 only; on resnet18 it raises ValueError that names "head+fpn+backbone", which in turn
        stays refused on resnet50): the whole ResNet-50 detector -- nothing is frozen, 189 tensors train.  A forward in train mode packs the
        image (nets.pack_image) and runs the stem (csrc/stem_train.hip, frozen statistics), res2 .. res5, the FPN and the head as one
        autograd node; no trunk engine is built or read.  res2.0 forms its input gradient, which is the stem's upstream gradient.  Frozen
        statistics only: trunk_bn must be "frozen".

        "head+fpn+res5+res4+res3" (ResNet-50 only; on resnet18 it raises ValueError that names "head+fpn+layer4+layer3+layer2"): one stage
        further down -- backbone.0 .. backbone.4 (the stem and res2) stop requiring grad; backbone.5 (four Bottlenecks of width 128, 39
        tensors), backbone.6 (57), backbone.7 (30), fpn (10) and head (20) train: 156 tensors.  A forward in train mode takes C2 from the
        trunk engine's forward_c2 (keyed on the frozen backbone tensors only; the engine stops after res2, so no stale C3, C4 or C5 is
        computed), then runs res3, res4, res5, the FPN and the head on the HIP training kernels as one autograd node.  Frozen statistics only:
        trunk_bn must be "frozen".

        None (default): forward-only on the fused inference engine, as always.  "head": fine-tune the DB head over a frozen trunk and
        FPN -- their parameters stop requiring grad, and a forward in train mode runs trunk + FPN on a separate features engine (built
        with fuse_fpn_head=0, rebuilt only when trunk / FPN weights change) and the head on the HIP training kernels, differentiable
        w.r.t. the head's parameters.  "head+fpn": fine-tune the FPN and the head over a frozen trunk -- the backbone's parameters stop
        requiring grad, and a forward in train mode runs the trunk on a trunk engine (fuse_fpn_head=0, keyed on the backbone tensors
        only: an optimizer step on FPN or head weights never rebuilds it), then the FPN and the head on the HIP training kernels as one
        autograd node, differentiable w.r.t. the FPN's ten live tensors and the head's twenty.  The trunk's BatchNorms use their running
        statistics (folded into the convolutions), as in "head" mode; backward through the trunk is not built.  eval() forwards keep
        the fused inference engine, rebuilt after updates of the trained tensors.  "head+fpn+layer4" (ResNet-18 only): also fine-tune
        the trunk's last stage -- backbone.0 .. backbone.6 stop requiring grad; backbone.7, fpn and head train.  A forward in train mode
        runs the trunk engine (keyed on the versions of the frozen backbone tensors only: an optimizer step on layer4, FPN or head never
        rebuilds it), takes C2..C4 from it -- the engine's own C5 comes from the layer4 weights it was built with and is ignored --, then
        runs layer4 on C4, the FPN and the head on the HIP training kernels as one autograd node.  layer4's BatchNorms, like the rest of
        the trunk's, normalise with their running statistics, which are never written.  "head+fpn+layer4+layer3" (ResNet-18 only): one stage
        further down -- backbone.0 .. backbone.5 stop requiring grad; backbone.6, backbone.7, fpn and head train.  The trunk engine is keyed
        on the frozen tensors only and gives C2 and C3 (its C4 and C5 are ignored); layer3, layer4, the FPN and the head run on the HIP
        training kernels as one autograd node.  layer4.0 forms its input gradient with the strided dgrad; dC4 is that plus the FPN's dC4.
        "head+fpn+layer4+layer3+layer2" (ResNet-18 only): the usual fine-tuning recipe of a detection trunk -- the stem and layer1
        (backbone.0 .. backbone.4) stop requiring grad; backbone.5 .. backbone.7, fpn and head train.  The trunk engine is keyed on the frozen
        tensors only and gives C2 (its C3, C4 and C5 are ignored); layer2, layer3, layer4, the FPN and the head run on the HIP training
        kernels as one autograd node.  dC3 is layer3.0's input gradient plus the FPN's dC3; layer2.0 forms no input gradient.
        "head+fpn+layer4+layer3+layer2+layer1" (ResNet-18 only): every residual stage -- only the stem (backbone.0, backbone.1) stops requiring
        grad; backbone.4 .. backbone.7, fpn and head train (87 tensors).  The trunk engine is keyed on the frozen tensors only and gives the
        pooled stem output (engine.DetectorEngine.forward_pool: the stem alone runs); layer1 .. layer4, the FPN and the head run on the HIP
        training kernels as one autograd node.  dC2 is layer2.0's input gradient plus the FPN's dC2; layer1.0 forms no input gradient.
        "head+fpn+backbone" (ResNet-18 only): the whole detector, as the reference's trainer hands every parameter to its optimizer -- nothing
        is frozen, 90 tensors train.  A forward in train mode packs the image (nets.pack_image) and runs the stem (csrc/stem_train.hip),
        layer1 .. layer4, the FPN and the head on the HIP training kernels as one autograd node; no trunk engine is built or read.  layer1.0
        forms its input gradient, which is the stem's upstream gradient; the stem's BatchNorm, like every trunk BatchNorm, normalises with
        its running statistics, which are never written -- unless trunk_bn="backbone" (above).  No gradient of the image is formed."""
        if trainable in _STAGE_MODES or trainable == _BACKBONE_MODE:
            if self.backbone_name != "resnet18":
                raise ValueError(f"trainable={trainable!r} is built for resnet18 only: {self.backbone_name} has Bottleneck blocks, and "
                                 "Bottleneck training is not built under this name (resnet50's last stage trains with trainable='head+fpn+res5')")
        elif trainable in _RES_MODES or trainable == _RES_WHOLE_MODE:
            if self.backbone_name != "resnet50":      # the refusal names ResNet-18's mode of the same depth
                k = (_RES_MODES + (_RES_WHOLE_MODE,)).index(trainable)
                raise ValueError(f"trainable={trainable!r} names ResNet-50's {_RES_MODE_NAMES[k][0]}; on {self.backbone_name} {_RES_MODE_NAMES[k][1]} "
                                 f"with trainable={(_STAGE_MODES + (_BACKBONE_MODE,))[k]!r}")
        elif trainable not in (None, "head", "head+fpn"):
            raise ValueError(f"trainable must be None, 'head' or 'head+fpn', got {trainable!r}")
        bn_mode = getattr(self, "trunk_bn", "frozen") if trunk_bn is None else trunk_bn
        if isinstance(bn_mode, str) and bn_mode == "bottleneck":
            if self.backbone_name != "resnet50" or trainable not in (_RES5_MODE, _RES4_MODE):
                raise ValueError(f"trunk_bn='bottleneck' with trainable={trainable!r} on {self.backbone_name}: " + _RES_BN_BUILT)
        elif (trainable in _RES_MODES or trainable == _RES_WHOLE_MODE) and not (isinstance(bn_mode, str) and bn_mode == "frozen"):
            who = ("res5 trains", "res4 and res5 train", "res3, res4 and res5 train", "res2, res3, res4 and res5 train",
                   "the stem and res2 .. res5 train")[(_RES_MODES + (_RES_WHOLE_MODE,)).index(trainable)]
            raise ValueError(f"trunk_bn={bn_mode!r} with trainable={trainable!r}: {who} with frozen-statistics BatchNorm only (trunk_bn='frozen') "
                             "under this spelling; " + _RES_BN_BUILT)
        if isinstance(bn_mode, (tuple, list)):
            bn_mode = tuple(bn_mode)
            fits = next((mode for stages, mode in _TRUNK_BN_STAGES.items() if stages == bn_mode), None)      # no hashing: any tuple may come
            if self.backbone_name != "resnet18" or fits is None or fits != trainable:
                raise ValueError(f"trunk_bn={bn_mode!r} with trainable={trainable!r} on {self.backbone_name}: " + _TRUNK_BN_BUILT)
        elif not isinstance(bn_mode, str) or bn_mode not in ("frozen", "batch", "trained", "backbone", "bottleneck"):
            raise ValueError(f"trunk_bn must be 'frozen' or 'batch' (or 'trained', 'backbone', 'bottleneck', or a tuple of stage names), got {bn_mode!r}")
        if bn_mode == "backbone" and (self.backbone_name != "resnet18" or trainable != _BACKBONE_MODE):
            raise ValueError(f"trunk_bn='backbone' with trainable={trainable!r} on {self.backbone_name}: " + _BACKBONE_BN_BUILT)
        if bn_mode == "trained" and (self.backbone_name != "resnet18" or trainable not in _TRAINED_BN_MODES):
            raise ValueError(f"trunk_bn='trained' with trainable={trainable!r} on {self.backbone_name}: " + _TRAINED_BN_BUILT)
        if bn_mode == "batch" and trainable != "head+fpn+layer4":
            raise ValueError(f"trunk_bn='batch' with trainable={trainable!r}: train-mode (batch-statistics) trunk BatchNorm is built for layer4 only, "
                             "that is for trainable='head+fpn+layer4' on resnet18; layer3, layer2, layer1 and the stem keep frozen statistics")
        self.trunk_bn = bn_mode
        self.trainable = trainable
        if trainable == "head":
            for p in list(self.backbone.parameters()) + list(self.fpn.parameters()):
                p.requires_grad_(False)
        elif trainable == "head+fpn":
            for p in self.backbone.parameters():
                p.requires_grad_(False)
        elif trainable in _STAGE_MODES or trainable in _RES_MODES:
            first = self._first_trained()
            for i in range(8):
                for p in self.backbone[i].parameters():
                    p.requires_grad_(i >= first)
            for p in list(self.fpn.parameters()) + list(self.head.parameters()):
                p.requires_grad_(True)
        elif trainable in (_BACKBONE_MODE, _RES_WHOLE_MODE):
            for p in self.parameters():
                p.requires_grad_(True)
        self._head_versions = None
        return self

    def _first_trained(self):
        """The first backbone module a stage mode trains: the mode at position k - 1 of _STAGE_MODES trains the top k residual stages,
        backbone.(8 - k) .. backbone.7, over the frozen backbone.0 .. backbone.(7 - k)."""
        if self.trainable in _RES_MODES:      # ResNet-50: res5 alone, res4 and res5, res3, res4 and res5, or all four stages
            return 7 - _RES_MODES.index(self.trainable)
        return 8 - (_STAGE_MODES.index(self.trainable) + 1)

    def _head_tensor_versions(self):
        tensors = list(self.head.parameters()) + list(self.head.buffers())
        if self.trainable == "head+fpn" or self.trainable in _STAGE_MODES or self.trainable in (_BACKBONE_MODE, _RES_WHOLE_MODE) + _RES_MODES:
            tensors += list(self.fpn.parameters())
        if self.trainable in (_BACKBONE_MODE, _RES_WHOLE_MODE):      # the four stages as in the layer1 mode, then the stem's three parameters and three buffers
            for i in (7, 6, 5, 4, 0, 1):
                tensors += list(self.backbone[i].parameters()) + list(self.backbone[i].buffers())
        if self.trainable in _STAGE_MODES or self.trainable in _RES_MODES:      # the stages the mode trains, from the last one down
            for i in range(7, self._first_trained() - 1, -1):
                tensors += list(self.backbone[i].parameters()) + list(self.backbone[i].buffers())
        return tuple(t._version for t in tensors)

    def trunk_engine(self):
        """The trunk engine of the "head+fpn" path (options fuse_fpn_head=0, see engine.DetectorEngine.forward_trunk)."""
        from . import engine as _e
        with self._engine_lock:
            # keyed on the backbone tensors' versions only (load_state_dict bumps them): FPN and head updates never rebuild it
            frozen = self.backbone.state_dict()
            if self.trainable in _STAGE_MODES or self.trainable in _RES_MODES:
                # the frozen tensors only: what the engine computes from the trained stages (stale weights) is never read -- its C5 in the
                # layer4 mode, C4 and C5 in the layer3 mode, all but C2 in the layer2 mode, all but the pooled stem output in the layer1 mode
                trained = tuple(f"{i}." for i in range(self._first_trained(), 8))
                frozen = {k: v for k, v in frozen.items() if not k.startswith(trained)}
            version = tuple(t._version for t in frozen.values())
            te = self.__dict__.get("_trunk_engine")
            if te is None or self.__dict__.get("_trunk_version") != version:
                te = _e.DetectorEngine(self.backbone_name, self.state_dict(), getattr(self, "_max_batch", None), options={"fuse_fpn_head": 0})
                self._trunk_engine, self._trunk_version = te, version
            return te

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
        state["_trunk_engine"] = None
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
        if self.trainable in ("head", "head+fpn", _BACKBONE_MODE, _RES_WHOLE_MODE) + _RES_MODES + _STAGE_MODES:
            if self.training:
                if self.trainable == _BACKBONE_MODE:
                    return self._forward_train_backbone(x)
                if self.trainable == _RES_WHOLE_MODE:
                    return self._forward_train_res_whole(x)
                if self.trainable in _RES_MODES:
                    return self._forward_train_res(x)
                if self.trainable in _STAGE_MODES:
                    return self._forward_train_trunk(x)
                return self._forward_train_head(x) if self.trainable == "head" else self._forward_train_head_fpn(x)
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

    def _forward_train_head_fpn(self, x):
        frozen = [n for n, p in self.backbone.named_parameters(prefix="backbone") if p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable='head+fpn'): {frozen[0]} requires grad, but backward through the trunk is not "
                               "implemented; only the FPN and the DB head train (set requires_grad_(False) on backbone)")
        for m in (self.fpn, self.head):
            if not next(m.parameters()).is_cuda:
                m.cuda()   # their own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        taps = self.trunk_engine().forward_trunk(x)   # new tensors per call: autograd may keep them
        out = self.fpn.forward_padded(taps, head=self.head)
        self.mark_dirty()   # the kernels updated the head's running statistics in place
        return out


    def _forward_train_trunk(self, x):
        """The train-mode forward of the stage modes: the frozen trunk engine up to the lowest trained stage, then the trained stages, the FPN and
        the head as one autograd node."""
        first = self._first_trained()
        k = 8 - first      # the stages that train: layer(5 - k) .. layer4
        frozen = [n for i in range(first) for n, p in self.backbone[i].named_parameters(prefix=f"backbone.{i}") if p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable={self.trainable!r}): {frozen[0]} requires grad, but backward below layer{5 - k} is not "
                               f"implemented; only {', '.join(f'layer{j}' for j in range(5 - k, 5))}, the FPN and the DB head train (set "
                               f"requires_grad_(False) on backbone.0 .. backbone.{first - 1})")
        for m in (*(self.backbone[i] for i in range(first, 8)), self.fpn, self.head):
            if not next(m.parameters()).is_cuda:
                m.cuda()   # their own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        # the engine's taps above the lowest trained stage's input come from the weights it was built with and are ignored; with every stage
        # trained the stem alone runs (forward_pool).  New tensors per call: autograd may keep them
        engine = self.trunk_engine()
        taps = [engine.forward_pool(x)] if k == 4 else engine.forward_trunk(x)[:4 - k]
        stages = {f"layer{j}": self.backbone[3 + j] for j in range(5 - k, 5)}
        # trunk_bn="batch" is the layer4 mode's alone and a tuple names the mode's own stages (set_trainable): the running statistics of those
        # stages move too; mark_dirty below covers them
        bn_mode = getattr(self, "trunk_bn", "frozen")
        if bn_mode == "trained":      # every stage the mode trains (set_trainable: layer1 at the lowest), on the node of that many stages
            bn_mode = tuple(stages)
        out = self.fpn.forward_padded(taps, head=self.head, trunk_batch_stats=bn_mode if isinstance(bn_mode, tuple) else bn_mode == "batch", **stages)
        self.mark_dirty()   # the kernels updated the head's running statistics in place
        return out

    def _forward_train_res(self, x):
        """The train-mode forward of ResNet-50's stage modes: the input of the lowest trained stage from the frozen trunk engine, then the
        trained stages, the FPN and the head as one autograd node.  What the engine computes from the trained stages comes from the weights
        it was built with and is ignored (its C5 in the res5 mode, C4 and C5 in the res4 mode) or never runs (forward_c2 stops at C2 in the
        res3 mode, forward_pool after the stem in the res2 mode)."""
        first = self._first_trained()
        stages = _RES_STAGES[first - 4:]
        frozen = [n for i in range(first) for n, p in self.backbone[i].named_parameters(prefix=f"backbone.{i}") if p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable={self.trainable!r}): {frozen[0]} requires grad, but backward below {stages[0].name} is not "
                               f"implemented; only {', '.join(f'{st.name} (backbone.{st.slot})' for st in stages)}, the FPN and the DB head train "
                               f"(set requires_grad_(False) on backbone.0 .. backbone.{first - 1}" +
                               (f", or pick trainable={_RES_WHOLE_MODE!r})" if first == 4 else ")"))
        for m in (*(self.backbone[st.slot] for st in stages), self.fpn, self.head):
            if not next(m.parameters()).is_cuda:
                m.cuda()   # their own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        engine = self.trunk_engine()      # new tensors per call: autograd may keep them
        taps = [engine.forward_pool(x)] if first == 4 else [engine.forward_c2(x)] if first == 5 else engine.forward_trunk(x)[:first - 4]
        # trunk_bn="bottleneck" (set_trainable: res5, or res4 and res5): the stages on the batch-statistics entries, their running buffers and
        # counters move too; mark_dirty covers them
        batch = {"res_batch_stats": True} if getattr(self, "trunk_bn", "frozen") == "bottleneck" else {}
        out = self.fpn.forward_padded(taps, head=self.head, **{st.name: self.backbone[st.slot] for st in stages}, **batch)
        self.mark_dirty()   # the kernels updated the head's running statistics in place
        return out

    def _forward_train_res_whole(self, x):
        """The train-mode forward of "head+fpn+res5+res4+res3+res2+stem": the image packed (nets.pack_image), then the stem, res2 .. res5, the
        FPN and the head as one autograd node; no trunk engine is built or read."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"DBNet(trainable={self.trainable!r}): the train-mode forward takes a float [n,3,H,W] tensor")
        frozen = [n for n, p in self.named_parameters() if not p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable={self.trainable!r}): {frozen[0]} does not require grad, but this mode trains every tensor "
                               "(pick a narrower mode with set_trainable to freeze a part)")
        for m in (self.backbone, self.fpn, self.head):
            if not next(m.parameters()).is_cuda:
                m.cuda()   # their own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        dev = next(self.head.parameters()).device
        image = pack_image(x if x.is_cuda else x.to(dev))   # no trunk engine: the stem runs on the training kernels too
        out = self.fpn.forward_padded([image], head=self.head, res5=self.backbone[7], res4=self.backbone[6], res3=self.backbone[5],
                                      res2=self.backbone[4], stem=(self.backbone[0], self.backbone[1]))
        self.mark_dirty()   # the kernels updated the head's running statistics in place
        return out

    def _forward_train_backbone(self, x):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("DBNet(trainable='head+fpn+backbone'): the train-mode forward takes a float [n,3,H,W] tensor")
        frozen = [n for n, p in self.named_parameters() if not p.requires_grad]
        if frozen:
            raise RuntimeError(f"DBNet(trainable='head+fpn+backbone'): {frozen[0]} does not require grad, but this mode trains every tensor "
                               "(pick a narrower mode with set_trainable to freeze a part)")
        for m in (self.backbone, self.fpn, self.head):
            if not next(m.parameters()).is_cuda:
                m.cuda()   # their own tensors are the kernels' operands (the optimizer keeps the same Parameter objects)
        dev = next(self.head.parameters()).device
        image = pack_image(x if x.is_cuda else x.to(dev))   # no trunk engine: the stem runs on the training kernels too
        # trunk_bn="backbone": the stem and the eight blocks on the batch-statistics entries; their running statistics move too (mark_dirty below)
        batch = {"trunk_batch_stats": _NODE_BN_STAGES[3], "stem_batch_stats": True} if getattr(self, "trunk_bn", "frozen") == "backbone" else {}
        out = self.fpn.forward_padded([image], head=self.head, layer4=self.backbone[7], layer3=self.backbone[6], layer2=self.backbone[5],
                                      layer1=self.backbone[4], stem=(self.backbone[0], self.backbone[1]), **batch)
        self.mark_dirty()   # the kernels updated the head's running statistics in place
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
