"""The vectorised latent-plan schedule without a GPU: `latent_plan_policy_restatement` (tacorl_amd/evaluation/vec_policy.py) in
fp64 against a literal per-environment transcription of the reference's rollout loop (tests/vec_rollout_util.reference_loop),
over callables standing in for the networks - re-plan steps, restart rows, the reset of a finished row, `plans=` overrides -
and the fp64 decoder restatement of the step_rows-against-act GPU case, which leaves out no case for the committed seed."""
import os

import numpy as np
import pytest
import torch

from tacorl_amd.evaluation.vec_policy import PlanClock, latent_plan_policy_restatement
from tests import vec_rollout_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, S, G, P, A, H, L = 4, 5, 2, 3, 2, 6, 2
D = torch.float64


def _nets(seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)  # noqa: E731
    wp, wx, wh, wa = rn(S + G, P), rn(P + S, H), rn(L, H, H) * 0.3, rn(H, A)

    def plan_fn(obs, goal, rows, t):
        return torch.tanh(torch.cat([obs, goal], dim=-1) @ wp + 0.01 * t)  # (the step enters: a plan made late differs)

    def decoder_fn(plan, obs, hidden, t):
        x = torch.cat([plan, obs], dim=-1) @ wx
        new = []
        for l in range(L):
            x = torch.relu(x + hidden[l] @ wh[l])
            new.append(x)
        return x @ wa + 0.001 * t, torch.stack(new)

    return plan_fn, decoder_fn


def _inputs(T, seed=1):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(R, S, generator=g, dtype=D) for _ in range(T)], [torch.randn(R, G, generator=g, dtype=D) for _ in range(T)])


# per row: the lengths of its consecutive episodes (a finished row is reset and starts the next one at once)
EPISODES = [[14], [5, 9], [3, 3, 8], [7, 7]]
T = 14


def _resets(episodes):
    out = {}
    for r, lens in enumerate(episodes):
        t = 0
        for n in lens[:-1]:
            t += n
            out.setdefault(t, []).append(r)
    return out


@pytest.mark.parametrize("plan_duration", [1, 3, 4, 16])
@pytest.mark.parametrize("with_plans", [False, True])
def test_restatement_equals_the_reference_loop_per_environment(plan_duration, with_plans):
    plan_fn, decoder_fn = _nets()
    obs, goals = _inputs(T)
    plans = None
    if with_plans:  # an external planner gives rows 1 and 2 a plan at steps 0 and 6; NaN rows are "not given"
        plans = {}
        for t in (0, 6):
            p = torch.full((R, P), float("nan"), dtype=D)
            p[1], p[2] = torch.tensor([0.1 * t, -0.2, 0.3], dtype=D), torch.tensor([0.5, 0.25 * t, -0.5], dtype=D)
            plans[t] = p
    got = latent_plan_policy_restatement(plan_fn, decoder_fn, obs, goals, R, plan_duration, torch.zeros(L, R, H, dtype=D),
                                         resets=_resets(EPISODES), plans=plans)
    assert len(got["actions"]) == T
    for r in range(R):
        want, planned = V.reference_loop(plan_fn, decoder_fn, obs, goals, r, EPISODES[r], plan_duration,
                                         torch.zeros(L, 1, H, dtype=D), plans=plans)
        assert len(want) == T
        assert [t for t in range(T) if r in got["replanned"][t]] == planned, r
        for t in range(T):
            # (fp64 on both sides; BLAS may add a 1-row product in another order than a 4-row one: 1e-12, where any
            # slip of the schedule - a stale plan, a hidden state not cleared - is O(1))
            assert torch.allclose(got["actions"][t][r], want[t], rtol=1e-12, atol=1e-12), (r, t)


def test_clock_replans_after_reset_and_every_duration():
    c = PlanClock(3, 3)
    seen = []
    for t in range(8):
        if t == 5:
            c.reset([2])
        if t == 6:
            c.reset(np.array([True, False, False]))
        due = c.due()
        seen.append(due)
        c.tick(set(due))
    assert seen == [[0, 1, 2], [], [], [0, 1, 2], [], [2], [0, 1], []]
    with pytest.raises(IndexError):
        c.reset([3])
    with pytest.raises(ValueError):
        PlanClock(0, 3)


@pytest.mark.parametrize("H_", [72, 2048])
def test_decoder_restatement_leaves_out_no_case_for_the_committed_seed(H_):
    pb = V.decoder_problem(H_)
    out = V.decoder_rollout64(pb)
    left = torch.stack(out["left_out"])
    assert left.shape == (V.STEPS, V.ROWS, 7) and int(left.sum()) == 0, left.nonzero().tolist()
    # the heads' bound is small against the heads: a comparison inside it says something
    rel = max((e.max() / h.abs().max()).item() for e, h in zip(out["head_err"], out["heads"]))
    print(f"H {H_}: worst head bound / max |head| = {rel:.3g}, smallest gap / bound margin ok")
    assert rel < 1e-2
    # row 1 restarts at step 2: its hidden state there does not depend on steps 0 and 1
    pb2 = dict(pb, emb=[e.clone() for e in pb["emb"]])
    pb2["emb"][0][1] += 1.0
    out2 = V.decoder_rollout64(pb2)
    assert not torch.equal(out["heads"][1][1], out2["heads"][1][1]) and torch.equal(out["heads"][2][1], out2["heads"][2][1])
    assert torch.equal(out["heads"][1][0], out2["heads"][1][0])


def test_rollout_fixtures_load_with_the_documented_shapes():
    """tools/gen_latent_plan_rollout_golden.py: get_dist's mean and std, one sample with its draw, three act steps with their
    two draws each from a cleared hidden state, the final hidden state (and the deterministic plan of the D4RL TACORL)."""
    from tests.d4rl_cfg import D4rlGolden
    from tests.golden_util import Golden

    for g, n, A, E in ((Golden("rollout_playlmp"), 2, 7, 32), (D4rlGolden("rollout_d4rl"), 3, 8, 29)):
        z, tape = g.z, g.tape(0)
        assert g.cfg["B"] == n and [k for k, _ in tape] == ["normal"] + ["rand"] * 6
        assert tape[0][1].shape == (n, 16)
        Da = A - 1 if A == 7 else A
        for t in range(3):
            assert tape[1 + 2 * t][1].numel() == n * Da * 10 and tape[2 + 2 * t][1].numel() == n * Da
        for k in ("normal_mean", "normal_std", "plan_sampled"):
            assert z[k].shape == (n, 16) and np.isfinite(z[k]).all()
        assert (z["normal_std"] > 0).all() and (np.abs(z["plan_sampled"]) <= 1).all()
        assert z["actions"].shape == (3, n, 1, A) and z["hidden"].shape == (2, n, 2048)
        batch = g.batch(0)
        if A == 7:
            assert z["pp_state"].shape == (n, 32) and z["pp_goal"].shape == (n, 32) and z["ad_state"].shape == (3, n, E)
            assert batch["states"]["rgb_static"].shape[:2] == (n, g.cfg["T"]) and set(np.unique(z["actions"][..., -1])) <= {-1.0, 1.0}
        else:
            assert z["plan"].shape == (n, 16) and batch["observations"].shape == (n, g.cfg["T"], E)
        assert all(tuple(s) == tuple(p.shape) for s, p in zip(g.shapes, g.params().values()))


@pytest.mark.parametrize("H_", [72, 2048])
def test_cross_path_bounds_hold_for_two_fp32_orders_and_catch_an_uncleared_row(H_):
    """The comparison tests/test_vec_policy_gpu.py makes between step_rows and act, on two fp32 paths in plain torch that sum
    in different orders: every layer's and the heads' difference sits inside vec_rollout_util.cross_path_bounds over all five
    steps; a path that does not clear row 1 at step 2 exceeds the bound of that row there - by more than 10 x - while the
    rows that do not restart stay inside."""
    pb = V.decoder_problem(H_)
    L = pb["L"]
    for fault in (False, True):
        ha = [torch.zeros(pb["R"], H_) for _ in range(L)]
        hb = [torch.zeros(pb["R"], H_) for _ in range(L)]
        for t in range(pb["steps"]):
            heads_a, na = V.decoder_step32(pb, t, ha, split=1)
            heads_b, nb = V.decoder_step32(pb, t, hb, clear=not (fault and t == 2), split=7)
            ref_a = V.decoder_step64(pb, t, ha, own_h=na)
            ref_b = V.decoder_step64(pb, t, hb, own_h=nb)
            lb, hbound = V.cross_path_bounds(pb, t, ref_a, ref_b, ha, hb, na, nb)
            ratios = [((na[l].double() - nb[l].double()).abs() / lb[l]).max(dim=1).values for l in range(L)]
            if fault and t == 2:
                assert ratios[0][1].item() > 10.0, ratios[0]
                assert max(ratios[0][0].item(), ratios[0][2].item()) <= 1.0
                break
            assert all(bool((r <= 1.0).all()) for r in ratios), (t, ratios)
            assert bool(((heads_a.double() - heads_b.double()).abs() <= hbound).all()), t
            ha, hb = na, nb
