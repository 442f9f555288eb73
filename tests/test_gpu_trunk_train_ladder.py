"""The depths of the trunk training node against each other on the GPU: one loss step of layer4 -> FPN -> head, layer3 -> .., layer2 -> ..,
layer1 -> .. and stem -> .. on the chain of tests/test_gpu_stem_train.py (a 96 x 64 image: pooled tap 24 x 16, C2 24 x 16, C3 12 x 8, C4 6 x 4,
C5 3 x 2, n = 2), each depth on the taps the stages below it produce (forward_stem_padded, forward_layer1..3_padded) and from the same saved
head state.  A depth that starts one stage lower computes the same C2 .. C5 from the same bits, and the parameter gradients of a block do not
depend on whether its dx is formed, so the two output maps and every gradient that two adjacent depths share must be the same bits: 45 (15 of
layer4, 10 of the FPN, 20 of the head), 60, 75 and 87 tensors.  The stem depth against the layer1 depth is also asserted, with the fp64
reference, in tests/test_gpu_stem_train.py; the other pairs only here.  The layer4 depth with `trunk_batch_stats=True` and layer4 in eval()
mode runs the frozen path of the batch-statistics entries and must give the bits of the layer4 depth without the flag."""
import copy

import pytest
import torch

import test_gpu_stem_train as st
from vtd_amd import nets, training

DEPTHS = ("layer4", "layer3", "layer2", "layer1", "stem")
SHARED = {("layer4", "layer3"): 45, ("layer3", "layer2"): 60, ("layer2", "layer1"): 75, ("layer1", "stem"): 87}

_RUNS = {}


def _ladder():
    """{depth: (probability, threshold, the gradients from the lowest trained stage up: stem, layer1 .. layer4, FPN, head)}, and "layer4-bn",
    computed once."""
    if _RUNS:
        return _RUNS
    stem, l1, l2, l3, l4, fpn, head, _, targets, image = st._chain_setup()
    state = copy.deepcopy(head.state_dict())
    poolp = nets.forward_stem_padded(stem[0], stem[1], image)
    c2p = nets.forward_layer1_padded(l1, poolp)
    c3p = nets.forward_layer2_padded(l2, c2p)
    c4p = nets.forward_layer3_padded(l3, c3p)
    assert poolp.shape == (2, 26, 18, 64) and c2p.shape == (2, 26, 18, 64) and c3p.shape == (2, 14, 10, 128) and c4p.shape == (2, 8, 6, 256)
    tgt = {k: v.cuda() for k, v in targets.items()}
    calls = {
        "layer4": (lambda: fpn.forward_padded([c2p, c3p, c4p], head=head, layer4=l4), (l4,)),
        "layer4-bn": (lambda: fpn.forward_padded([c2p, c3p, c4p], head=head, layer4=l4, trunk_batch_stats=True), (l4,)),
        "layer3": (lambda: fpn.forward_padded([c2p, c3p], head=head, layer4=l4, layer3=l3), (l3, l4)),
        "layer2": (lambda: fpn.forward_padded([c2p], head=head, layer4=l4, layer3=l3, layer2=l2), (l2, l3, l4)),
        "layer1": (lambda: fpn.forward_padded([poolp], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1), (l1, l2, l3, l4)),
        "stem": (lambda: fpn.forward_padded([image], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1, stem=(stem[0], stem[1])),
                 (stem, l1, l2, l3, l4)),
    }
    for name, (call, trained) in calls.items():
        head.load_state_dict(state)
        for m in (stem, l1, l2, l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        l4.train(name != "layer4-bn")      # eval(): the frozen path of the batch-statistics entries
        out = call()
        training.detection_loss(out, tgt)["loss"].backward()
        grads = [p.grad.clone() for m in trained for p in m.parameters()] + [p.grad.clone() for p in fpn.live_parameters()] + \
            [p.grad.clone() for p in head.parameters()]
        assert all(p.grad is None for m in (stem, l1, l2, l3, l4) if m not in trained for p in m.parameters())
        _RUNS[name] = (out["probability"].detach().clone(), out["threshold"].detach().clone(), grads)
    l4.train()
    return _RUNS


def _differing(a, b, shared):
    """The indices (0, 1: the maps; 2 ..: the shared gradients, the shallower depth's order) at which two runs differ, with the largest
    absolute difference of each."""
    pa, pb = [a[0], a[1]] + a[2][-shared:], [b[0], b[1]] + b[2][-shared:]
    assert len(pa) == len(pb) == 2 + shared
    return {i: float((x.double() - y.double()).abs().max()) for i, (x, y) in enumerate(zip(pa, pb)) if not torch.equal(x, y)}


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(SHARED), ids=["-".join(p) for p in SHARED])
def test_adjacent_depths_give_the_same_bits(hip, pair):
    runs = _ladder()
    upper, lower = runs[pair[0]], runs[pair[1]]
    shared = SHARED[pair]
    assert len(upper[2]) == shared and len(lower[2]) > shared
    assert float(upper[0].max()) > 0 and all(float(g.abs().max()) > 0 for g in upper[2])
    diff = _differing(upper, lower, shared)
    print(f"MEASURED ladder {pair[0]} vs {pair[1]}: {2 + shared} tensors compared, {len(diff)} differ {diff}")
    assert not diff, diff


@pytest.mark.gpu
def test_frozen_path_of_the_batch_statistics_node_gives_the_same_bits(hip):
    runs = _ladder()
    diff = _differing(runs["layer4"], runs["layer4-bn"], 45)
    print(f"MEASURED ladder layer4 vs layer4 with trunk_batch_stats in eval(): 47 tensors compared, {len(diff)} differ {diff}")
    assert len(runs["layer4-bn"][2]) == 45 and not diff, diff
