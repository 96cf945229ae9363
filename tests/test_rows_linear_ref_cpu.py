"""tests/rows_linear_ref.py on its own (no GPU): an fp32 evaluation of the restatement - torch's CPU kernels, another
summation order than the HIP kernel's - sits inside the a-priori bound, and the bound is at least FAULT_RATIO below each of
three faults injected into the restatement, so tests/test_rows_linear_gpu.py would see them."""
import pytest
import torch

from tests import rows_linear_ref as RL


@pytest.mark.parametrize("K1,K2", RL.SHAPES_K + [(2048, 2048)])
def test_fp32_evaluation_sits_inside_the_bound(K1, K2):
    p = RL.problem(5, K1, K2, 182, seed=K1 + K2, flag_rows=(1,) if K2 else ())
    for act in (RL.ACT_NONE, RL.ACT_RELU):
        y64, scale = RL.restate(p, act)
        y32, _ = RL.restate(p, act, dtype=torch.float32)
        assert bool(((y32.double() - y64).abs() <= RL.bound(p, scale)).all())


@pytest.mark.parametrize("K1,K2", [(45, 72), (72, 72), (257, 259)])
@pytest.mark.parametrize("fault", ["tail", "row", "b2"])
def test_bound_is_far_below_each_fault(K1, K2, fault):
    """At the small shapes, where the kernel's scalar head and tail do run.  (The bound grows with K^2 for operands of one
    scale, a single product does not: at K1 = K2 = 2048 one dropped element is 1.08 x the bound and the 'row' fault 112 x;
    that shape's rows are whole 16-byte words, so it has no head and no tail to drop.)"""
    p = RL.problem(3, K1, K2, 7, seed=11 + K1)
    y, scale = RL.restate(p, RL.ACT_NONE)
    bad, _ = RL.restate(p, RL.ACT_NONE, fault=fault)
    ratio = ((bad - y).abs() / RL.bound(p, scale)).max().item()
    print(f"fault {fault} at K = ({K1}, {K2}): {ratio:.3g} x the bound")
    assert ratio >= RL.FAULT_RATIO, ratio


def test_flagged_rows_count_as_zeros_and_faults_touch_only_their_target():
    p = RL.problem(3, 48, 72, 7, seed=3, flag_rows=(2,))
    y, _ = RL.restate(p, RL.ACT_NONE)
    q = dict(p, x2=None, w2=None)
    y_no_x2, _ = RL.restate(q, RL.ACT_NONE)
    assert torch.equal(y[2], y_no_x2[2]) and not torch.equal(y[0], y_no_x2[0])
    bad, _ = RL.restate(p, RL.ACT_NONE, fault="b2")
    n = RL.fault_neuron(p)
    keep = [i for i in range(7) if i != n]
    assert torch.equal(bad[:, keep], y[:, keep]) and not torch.equal(bad[:, n], y[:, n])
    bad, _ = RL.restate(p, RL.ACT_NONE, fault="row")
    assert torch.equal(bad[1:], y[1:]) and not torch.equal(bad[0], y[0])
