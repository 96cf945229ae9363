"""What the checks of tests/test_rows_policy_gpu.py can see, shown on the restatement alone (tests/rows_policy_ref.py): every
row of every shape used there has an fp64 logit gap far above the logits' bounds - so the gripper column is compared exactly
and no row is skipped - and each seeded fault exceeds the a-priori bound of the place it lands in by FAULT_RATIO."""
import pytest
import torch

from tests import rows_policy_ref as RP


def _grip_cases():
    seen = []
    for shape, head, _ in RP.cases():
        if head[1] and (shape, head) not in seen:
            seen.append((shape, head))
    return seen


@pytest.mark.parametrize("shape,head", _grip_cases())
def test_every_row_has_a_logit_gap_far_above_the_bounds(shape, head):
    """All 64 rows of the seeded problem (every R of the GPU test is a prefix of them): |l1 - l0| > GAP_RATIO x (bound of l0 +
    bound of l1) in fp64.  The share of rows a gripper comparison would have to skip is zero by construction."""
    p = RP.problem(shape, head)
    m = RP.gap_margin(p, RP.MAX_ROWS)
    print(f"{shape} {head}: smallest logit gap / summed bounds = {m.min().item():.3g}")
    assert bool((m > RP.GAP_RATIO).all()), m.min().item()
    a = RP.restate(p, RP.MAX_ROWS)["action"]
    if shape in RP.SHAPES:  # (behind four layers the rows' hidden states are alike: the configured shape decides one way)
        assert bool((a[:, -1] == 1).any()) and bool((a[:, -1] == -1).any())  # both decisions occur


def test_fp32_chain_sits_inside_the_bounds():
    """The same chain evaluated by plain fp32 torch, layer by layer on its own inputs, is inside the bounds (they are not
    tighter than fp32 arithmetic allows) and gives the same gripper column."""
    for shape in RP.SHAPES:
        for head in RP.HEADS:
            p = RP.problem(shape, head)
            f = RP.restate(p, 17, dtype=torch.float32)
            for l in range(p["L"]):
                ref, bnd = RP.layer_ref(p, l, f["h"][l])
                assert bool(((f["y"][l].double() - ref).abs() <= bnd).all()), (shape, head, l)
            ref, bnd, _, _ = RP.action_ref(p, f["h"][-1])
            Ac = p["Ac"]
            assert bool(((f["action"][:, :Ac].double() - ref[:, :Ac]).abs() <= bnd).all())
            assert torch.equal(f["action"][:, Ac:].double(), ref[:, Ac:])


@pytest.mark.parametrize("shape", RP.SHAPES + [RP.REAL_SHAPE])
@pytest.mark.parametrize("fault", ["logstd", "grip_sign", "subgoal_row", "tail", "bias"])
def test_seeded_faults_exceed_the_bound(shape, fault):
    p = RP.problem(shape, RP.HEADS[0])
    R, L, Ac = 3, p["L"], p["Ac"]
    clean, bad = RP.restate(p, R), RP.restate(p, R, fault=fault)
    if fault == "grip_sign":
        assert bool((bad["action"][:, -1] != clean["action"][:, -1]).all())
        return
    if fault == "logstd":      # lands in action column 0; checked on the head's own (clean) input
        ref, bnd, _, _ = RP.action_ref(p, clean["h"][-1])
        ratio = ((bad["action"][:, :Ac] - ref[:, :Ac]).abs() / bnd)[:, 0].min()
    elif fault in ("subgoal_row", "tail"):  # lands in layer 0's output; the check feeds the layer the rows it was given
        ref, bnd = RP.layer_ref(p, 0, clean["h"][0])
        err = (bad["y"][0] - ref).abs() / bnd
        ratio = err[0].max() if fault == "subgoal_row" else err.max(dim=1).values.min()
    else:                      # 'bias': one neuron of the last hidden layer, every row
        ref, bnd = RP.layer_ref(p, L - 1, clean["h"][L - 1])
        ratio = ((bad["y"][L - 1] - ref).abs() / bnd)[:, RP.fault_neuron(p, L - 1)].min()
    print(f"{shape} {fault}: {ratio.item():.3g} x the bound")
    assert ratio.item() > RP.FAULT_RATIO, ratio.item()
