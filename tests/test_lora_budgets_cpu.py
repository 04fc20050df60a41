"""The error budgets of tests/lora_ref.py, proved on the CPU: every fp32 restatement of the LoRA kernels stays at or below 0.6 of
its budget on every shape of the table, and every listed mutation (the realistic bugs of exactly this code) leaves the budget on
every shape where it applies.  The factors are printed (pytest -s)."""
import pytest
import torch

from tests import lora_ref as lr


@pytest.mark.parametrize("kind", lr.KINDS)
def test_restatement_stays_inside_and_mutations_leave(kind):
    torch.manual_seed(0)
    top, low = 0.0, {m: float("inf") for m in lr.MUTATIONS}
    for (M, N, K, R) in lr.SHAPES:
        inp = lr.grads_inputs(M, N, K, R, kind)
        for acc in (False, True):
            ref = lr.grads_reference(inp, acc)
            r = lr.grads_ratio(lr.grads_restatement(inp, acc), ref)
            top = max(top, r)
            assert r <= 0.6, (kind, M, N, K, R, acc, r)
            for mut in lr.MUTATIONS:
                if not lr.applies(mut, M, N, K, R, acc):
                    continue
                f = lr.grads_ratio(lr.grads_restatement(inp, acc, mut), ref)
                low[mut] = min(low[mut], f)
                assert f > 1.0, (kind, mut, M, N, K, R, acc, f)
    print(f"\nlora grads {kind}: restatement at most {top:.3f} of the budget; smallest factor per mutation: "
          + ", ".join(f"{m} {v:.3g}" for m, v in low.items()))


def test_merge_restatement_and_mutations():
    top, low = 0.0, {m: float("inf") for m in lr.MERGE_MUTATIONS}
    for (N, K, R) in lr.MERGE_SHAPES:
        inp = lr.merge_inputs(N, K, R)
        ref, budget = lr.merge_reference(inp)
        r = lr.worst((lr.merge_restatement(inp).double() - ref).abs(), budget)[0]
        top = max(top, r)
        assert r <= 0.6, (N, K, R, r)
        for mut in lr.MERGE_MUTATIONS:
            f = lr.worst((lr.merge_restatement(inp, mut).double() - ref).abs(), budget)[0]
            low[mut] = min(low[mut], f)
            assert f > 1.0, (mut, N, K, R, f)
    print(f"\nlora merge: restatement at most {top:.3f} of the budget; smallest factor per mutation: "
          + ", ".join(f"{m} {v:.3g}" for m, v in low.items()))


def test_table_covers_the_slab_edges():
    assert lr.SLAB == __import__("reed_amd.ops", fromlist=["ops"]).LORA_UV_ROWS
    assert set(lr.MS) == {16, lr.SLAB - 1, lr.SLAB, 2 * lr.SLAB + 16}
    assert {(N, K) for _, N, K, _ in lr.SHAPES} == {(128, 128), (384, 128), (128, 512)} and {R for *_, R in lr.SHAPES} == {8, 16, 64}
