"""Host logic of the Transformer recogniser's pipelined path, without a device: how queued tickets are cut into passes
(engine.plan_passes) and when a pinned buffer may be handed out again (engine.PinnedPool)."""
import torch

from vtd_amd.engine import PinnedPool, plan_passes


def test_tickets_merge_into_passes_of_pass_tickets():
    assert plan_passes([3, 2, 4, 1, 5], 2, 16) == [
        [(0, 0, 3, 0), (1, 0, 2, 3)],
        [(2, 0, 4, 0), (3, 0, 1, 4)],
        [(4, 0, 5, 0)],
    ]


def test_a_ticket_larger_than_max_crops_is_cut_across_passes():
    assert plan_passes([4, 20], 2, 8) == [
        [(0, 0, 4, 0), (1, 0, 4, 4)],
        [(1, 4, 8, 0)],
        [(1, 12, 8, 0)],
    ]
    # cuts fall inside tickets too; a group that fills its last pass exactly leaves no empty pass behind
    assert plan_passes([5, 7, 2], 3, 6) == [
        [(0, 0, 5, 0), (1, 0, 1, 5)],
        [(1, 1, 6, 0)],
        [(2, 0, 2, 0)],
    ]
    assert plan_passes([4, 4, 3], 2, 8) == [[(0, 0, 4, 0), (1, 0, 4, 4)], [(2, 0, 3, 0)]]


def test_every_row_is_staged_once_within_max_crops():
    rows, max_crops = [7, 0, 31, 1, 12, 40, 3], 10
    passes = plan_passes(rows, 3, max_crops)
    seen = {i: [] for i in range(len(rows))}
    for runs in passes:
        off = 0
        for i, first, n, at in runs:
            assert at == off and n > 0   # runs are packed back to back from offset 0
            seen[i] += range(first, first + n)
            off += n
        assert 0 < off <= max_crops
        assert len({i for i, *_ in runs}) == len(runs)   # one run per ticket per pass
    assert all(seen[i] == list(range(r)) for i, r in enumerate(rows))
    # a group never shares a pass with the next one
    assert all(len({i // 3 for i, *_ in runs}) == 1 for runs in passes)


def test_one_pass_per_ticket_without_merging():
    assert plan_passes([3, 0, 5, 1], 1, 16) == [[(0, 0, 3, 0)], [(2, 0, 5, 0)], [(3, 0, 1, 0)]]
    assert plan_passes([], 2, 16) == []


def test_pinned_pool_waits_for_the_event_before_a_buffer_is_handed_out_again():
    pool = PinnedPool()
    spare, buf = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32)
    pool.release(spare, None)   # (no GPU work ever touched it)
    seen = []

    class _Event:
        def synchronize(self):
            got = pool.take((4, 3))
            seen.append(got is spare)   # `buf` is not in the pool while its event is waited for
            pool.release(got, None)

    pool.release(buf, _Event())
    assert seen == [True]
    assert pool.take((4, 3)) is buf and pool.take((4, 3)) is spare
