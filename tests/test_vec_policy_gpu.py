"""The vectorised latent-plan rollout on the GPU: ActionDecoderLogistic.step_rows against `act` on one single-row decoder per
row, LatentPlanPolicy's per-row schedule against the same rows run alone, the goldens recorded from the reference
(rollout_tacorl of oracle/gen_golden.py; rollout_playlmp / rollout_d4rl of tools/gen_latent_plan_rollout_golden.py) through
the policy and through the new rollout surfaces, and rollout_episodes on four fake environments whose episodes end at
different steps."""
import numpy as np
import pytest
import torch

from tests import cfg_util as C
from tests import d4rl_cfg as K
from tests import vec_rollout_util as V
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def G():
    from tacorl_amd import _lib

    return _lib.lib().tacorl_rows_linear2_group()


# ------------------------------------------------------------------------------------------ step_rows against act
def _decoder(pb):
    from tacorl_amd.networks.action_decoder import ActionDecoderLogistic

    ad = ActionDecoderLogistic(DEV, state_dim=pb["E"], latent_plan_dim=pb["P"], hidden_size=pb["H"], out_features=7, num_layers=pb["L"])
    for k, v in pb["W"].items():
        ad.blk.views[k].copy_(v)
    return ad


@pytest.mark.parametrize("H", [2048, 72])
def test_step_rows_against_act(H):
    """act is the yardstick: one single-row decoder per row, clear_hidden_state() where that row restarts.  Per step, every layer
    and the heads of both paths sit inside the layer's a-priori bound on the operands the path fed it
    (vec_rollout_util.decoder_step64), and the two paths' hidden states and heads differ by no more than the sum of both
    paths' a-priori bounds plus the weights' absolute values times the difference of what the layer was fed
    (vec_rollout_util.cross_path_bounds: restarted rows count as zeros on both sides, so a row that is not cleared has no
    allowance).  The sampled actions agree per (row, step, dimension) at 1e-4 relative (gripper: exactly), a case being left
    out only where the fp64 scores' two best are closer than twice the heads' bound, the sum of both paths' a-priori bounds."""
    pb = V.decoder_problem(H)
    R, L, NH = pb["R"], pb["L"], 3 * pb["Da"] * pb["K"] + 2
    ad = _decoder(pb)
    singles = [_decoder(pb) for _ in range(R)]
    state = ad.new_rows_state(R)
    plan = pb["plan"].to(DEV)
    cpu64 = lambda ts: [t.detach().double().cpu() for t in ts]  # noqa: E731
    h_rows = [torch.zeros(R, H, dtype=torch.float64) for _ in range(L)]
    h_act = [torch.zeros(R, H, dtype=torch.float64) for _ in range(L)]
    cases = left_out = 0
    worst = dict(layer=0.0, cross=0.0, heads=0.0, action=0.0)
    for t in range(pb["steps"]):
        emb, ra, rb = pb["emb"][t].to(DEV), pb["ra"][t].to(DEV), pb["rb"][t].to(DEV)
        a_rows = ad.step_rows(state, plan, emb, pb["restart"][t], noise=(ra, rb)).clone()
        new_rows = cpu64(state.hidden)
        heads_rows = state.heads[:, :NH].double().cpu()
        a_act, heads_act, new_act = [], [], [[] for _ in range(L)]
        for r, dec in enumerate(singles):
            if pb["restart"][t][r]:
                dec.clear_hidden_state()
            a_act.append(dec.act(plan[r: r + 1], emb[r: r + 1].unsqueeze(1), noise=(ra[r: r + 1], rb[r: r + 1]))[0, 0])
            heads_act.append(dec._act_heads[0, :NH].double().cpu())
            for l in range(L):
                new_act[l].append(dec.hidden_state[l, 0].double().cpu())
        a_act, heads_act = torch.stack(a_act).cpu(), torch.stack(heads_act)
        new_act = [torch.stack(v) for v in new_act]
        # each path against fp64 on its own operands
        ref_r = V.decoder_step64(pb, t, h_rows, own_h=new_rows)
        ref_a = V.decoder_step64(pb, t, h_act, own_h=new_act)
        for l in range(L):
            ratio = ((new_rows[l] - ref_r[4][l]).abs() / ref_r[5][l]).max().item()
            worst["layer"] = max(worst["layer"], ratio)
            assert ratio <= 1.0, (t, l, ratio)
        assert bool(((heads_rows - ref_r[0]).abs() <= ref_r[1]).all()) and bool(((heads_act - ref_a[0]).abs() <= ref_a[1]).all())
        lb, hb = V.cross_path_bounds(pb, t, ref_r, ref_a, h_rows, h_act, new_rows, new_act)
        for l in range(L):
            ratio = ((new_rows[l] - new_act[l]).abs() / lb[l]).max().item()
            worst["cross"] = max(worst["cross"], ratio)
            assert ratio <= 1.0, (t, l, ratio)
        ratio = ((heads_rows - heads_act).abs() / hb).max().item()
        worst["heads"] = max(worst["heads"], ratio)
        assert ratio <= 1.0, (t, ratio)
        skip = ref_a[3] < 2 * V.deciding_bound(pb, ref_r[1] + ref_a[1])
        cases, left_out = cases + skip.numel(), left_out + int(skip.sum())
        arm_err = (a_rows.cpu()[:, :-1] - a_act[:, :-1]).abs() / a_act[:, :-1].abs()
        grip_ok = a_rows.cpu()[:, -1] == a_act[:, -1]
        ok = torch.cat([arm_err <= 1e-4, grip_ok.unsqueeze(1)], dim=1) | skip
        worst["action"] = max(worst["action"], arm_err[~skip[:, :-1]].max().item())
        assert bool(ok.all()), (t, arm_err, skip)
        h_rows, h_act = new_rows, new_act
    print(f"H {H}: worst layer {worst['layer']:.3g}, hidden difference {worst['cross']:.3g} and heads difference {worst['heads']:.3g} of their bounds, actions {worst['action']:.3g} "
          f"relative; {left_out} of {cases} cases left out")
    assert left_out <= V.LEFT_OUT_CAP * cases


# ------------------------------------------------------------------------------------------ schedule
def _d4rl_tacorl(seed=0):
    torch.manual_seed(seed)
    lmp = K.build(K.playlmp_d4rl_cfg(latent=16, T=8, device=DEV, dropout_p=0.0))
    return K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=False, device=DEV)), lmp


def test_schedule_rows_equal_the_same_row_alone():
    """D4RL TACORL, R = G + 1, plan_duration 3, eight steps, plans and draws injected, row 2 reset after step 4: with the plan
    given and the vector observation used as the embedding the step is the rows kernel plus a per-row elementwise sampler,
    so every row's action sequence is bit-identical to that row run alone through an R = 1 policy."""
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy

    mod, _ = _d4rl_tacorl()
    mod.eval()
    R, T, P = G() + 1, 8, 16
    g = torch.Generator().manual_seed(5)
    obs = [torch.rand(R, 29, generator=g) * 2 - 1 for _ in range(T)]
    goal = torch.rand(R, 2, generator=g) * 2 - 1
    plans = [torch.tanh(torch.randn(R, P, generator=g)) for _ in range(T)]
    ra = [torch.rand(R, 8, 10, generator=g) for _ in range(T)]
    rb = [torch.rand(R, 8, generator=g) for _ in range(T)]

    def run(rows):
        pol = LatentPlanPolicy(mod, n_envs=len(rows), plan_duration=3)
        pol.reset()
        out, due = [], []
        for t in range(T):
            if t == 5 and 2 in rows:
                pol.reset([rows.index(2)])
            due.append([rows[i] for i in pol.clock.due()])
            pl = plans[t][rows] if len(rows) == 1 else plans[t][rows].to(DEV)  # (a host tensor: the plan source is skipped)
            out.append(pol.step(obs[t][rows], goal[rows], noise={"rand_a": ra[t][rows], "rand_b": rb[t][rows]}, plans=pl).clone().cpu())
        return out, due

    full, due = run(list(range(R)))
    assert due[0] == list(range(R)) and due[3] == list(range(R)) and due[5] == [2] and due[6] == [r for r in range(R) if r != 2]
    assert due[1] == due[2] == due[4] == [] and due[7] == []
    assert all(bool(torch.isfinite(a).all()) and a.shape == (R, 8) for a in full)
    for r in range(R):
        alone, _ = run([r])
        for t in range(T):
            assert torch.equal(alone[t][0], full[t][r]), (r, t)
    assert not torch.equal(full[5][2], full[5][1])


# ------------------------------------------------------------------------------------------ goldens
def test_golden_rollout_tacorl_through_the_policy(tmp_path):
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy
    from tacorl_amd.modules.tacorl.tacorl import TACORL

    g = Golden("rollout_tacorl")
    z, params = g.z, g.params()
    C.write_reference_run_dir(str(tmp_path), C.lmp_state_dict_from_tacorl(params))
    strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
    mod = TACORL(play_lmp_dir=str(tmp_path), compute_dtype="f32", image_dtype="f32",
                 **strip(C.tacorl_cfg(device=DEV, finetune_action_decoder=False)))
    mod.load_state_dict(params, strict=False)
    mod.eval()
    batch, tape = g.batch(0), g.tape(0)
    frame = lambda t: {c: v[:, t] for c, v in batch["states"].items()}  # noqa: E731
    pol = LatentPlanPolicy(mod, n_envs=2, plan_duration=16)
    pol.reset()
    a0 = pol.step(frame(0), batch["goal"], noise={"rand_a": tape[1][1], "rand_b": tape[2][1]})
    assert a0.shape == (2, 7) and _rel(pol.plan, z["plan"]) < 1e-4, _rel(pol.plan, z["plan"])
    pol.reset()
    plan_ref = torch.from_numpy(z["plan"])
    for t in range(3):
        a = pol.step(frame(t), batch["goal"], noise={"rand_a": tape[1 + 2 * t][1], "rand_b": tape[2 + 2 * t][1]}, plans=plan_ref)
        want = torch.from_numpy(z["actions"][t])[:, 0]
        assert torch.equal(a[:, -1].cpu(), want[:, -1]), t
        assert _rel(a[:, :-1], want[:, :-1]) < 1e-3, (t, _rel(a[:, :-1], want[:, :-1]))
    assert _rel(torch.stack(list(pol.hidden)), z["hidden"]) < 1e-4
    # cat_output=False: the per-camera dict whose concatenation is the default
    cams = mod.action_decoder_modalities
    d = mod.perceptual_encoder.get_state_from_observation(frame(0), cams, cat_output=False)
    assert sorted(d) == sorted(cams)
    assert torch.equal(torch.cat([d[c] for c in cams], dim=-1), mod.perceptual_encoder.get_state_from_observation(frame(0), cams))


def test_golden_rollout_playlmp_through_the_new_surfaces():
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy

    g = Golden("rollout_playlmp")
    z = g.z
    mod = K.build(C.playlmp_cfg(cams=sorted(g.cams), latent=g.cfg["latent"], T=16, device=DEV))
    missing, unexpected = mod.load_state_dict(g.params(), strict=False)
    assert not unexpected, unexpected
    mod.eval()
    batch, tape = g.batch(0), g.tape(0)
    frame = lambda t: {c: v[:, t] for c, v in batch["states"].items()}  # noqa: E731
    cams = mod.plan_proposal_obs_modalities
    pe = mod.perceptual_encoder
    emb = pe.get_state_from_observation(observation=frame(0), modalities=cams, cat_output=False)
    assert isinstance(emb, dict) and sorted(emb) == sorted(cams)
    pp_state = torch.cat([emb[c] for c in cams], dim=-1)
    assert torch.equal(pp_state, pe.get_state_from_observation(frame(0), cams))
    pp_goal = mod.goal_encoder(pe.get_state_from_observation(observation=batch["goal"], modalities=mod.plan_proposal_goal_modalities))
    assert _rel(pp_state, z["pp_state"]) < 1e-4 and _rel(pp_goal, z["pp_goal"]) < 1e-4
    dist = mod.plan_proposal.get_dist(state_emb=pp_state, goal_emb=pp_goal)
    assert _rel(dist.normal_mean, z["normal_mean"]) < 1e-4 and _rel(dist.normal_std, z["normal_std"]) < 1e-4
    assert _rel(dist.stddev, z["normal_std"]) < 1e-4 and _rel(dist.mean, np.tanh(z["normal_mean"])) < 1e-4
    assert not dist.normal_mean.requires_grad
    assert _rel(dist.sample(noise=tape[0][1]), z["plan_sampled"]) < 1e-4
    assert _rel(dist.rsample(noise=tape[0][1]), z["plan_sampled"]) < 1e-4
    # the whole first plan and three decoder steps through the policy
    pol = LatentPlanPolicy(mod, n_envs=2, plan_duration=16)
    pol.reset()
    for t in range(3):
        a = pol.step(frame(t), batch["goal"], noise={"plan_eps": tape[0][1], "rand_a": tape[1 + 2 * t][1], "rand_b": tape[2 + 2 * t][1]})
        if t == 0:
            assert _rel(pol.plan, z["plan_sampled"]) < 1e-4
        want = torch.from_numpy(z["actions"][t])[:, 0]
        assert torch.equal(a[:, -1].cpu(), want[:, -1]) and _rel(a[:, :-1], want[:, :-1]) < 1e-3, (t, _rel(a[:, :-1], want[:, :-1]))
    assert _rel(torch.stack(list(pol.hidden)), z["hidden"]) < 1e-4
    # the reference's own call sequence (act / clear_hidden_state on the module's container)
    mod.action_decoder.clear_hidden_state()
    plan = torch.from_numpy(z["plan_sampled"]).to(DEV)
    a = mod.action_decoder.act(latent_plan=plan, perceptual_emb=pe.get_state_from_observation(frame(0), mod.action_decoder_modalities).unsqueeze(1),
                               noise=(tape[1][1], tape[2][1]))
    assert _rel(a[:, 0, :-1], z["actions"][0][:, 0, :-1]) < 1e-3


def test_golden_rollout_d4rl_through_the_new_surfaces():
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy
    from tacorl_amd.modules.cem import CEMOptimizer, cem_restatement, n_elite_of

    g = K.D4rlGolden("rollout_d4rl")
    z = g.z
    lmp = K.build(K.playlmp_d4rl_cfg(latent=g.cfg["latent"], T=g.cfg["T"], device=DEV, dropout_p=0.0))
    mod = K.build(K.tacorl_d4rl_cfg(play_lmp=lmp, finetune_action_decoder=False, device=DEV))
    P = g.params()
    missing, unexpected = mod.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    lmp.plan_proposal.load_state_dict({k[len("actor."):]: v for k, v in P.items() if k.startswith("actor.")})
    mod.eval()
    batch, tape = g.batch(0), g.tape(0)
    obs, goal = batch["observations"].to(DEV), batch["goal"].to(DEV)
    dist = lmp.plan_proposal.get_dist(state_emb=obs[:, 0], goal_emb=goal)
    assert _rel(dist.normal_mean, z["normal_mean"]) < 1e-4 and _rel(dist.normal_std, z["normal_std"]) < 1e-4
    assert _rel(dist.sample(noise=tape[0][1]), z["plan_sampled"]) < 1e-4
    one = lmp.plan_proposal.get_dist(state_emb=obs[1, 0], goal_emb=goal[1]).sample(noise=tape[0][1][1])  # (29,), (2,): one row
    assert one.shape == (16,) and _rel(one, z["plan_sampled"][1]) < 1e-4
    og = torch.cat([obs[:, 0], goal], dim=-1)
    plan, lp = mod.actor.get_actions(og, deterministic=True, reparameterize=False)
    assert plan.shape == (3, 16) and float(lp.abs().max()) == 0.0 and _rel(plan, z["plan"]) < 1e-4
    p1, _ = mod.actor.get_actions(og[2], deterministic=True)
    assert p1.shape == (16,) and _rel(p1, z["plan"][2]) < 1e-4
    assert mod.actor.action_dim == 16 and mod.actor.discrete_gripper is False
    ps, lps = mod.actor.get_actions(og, deterministic=False, noise={"eps": tape[0][1]})
    assert lps.shape == (3, 1) and bool(torch.isfinite(lps).all()) and bool((ps.abs() <= 1).all())
    # three decoder steps of the golden plan through the policy and through act
    pol = LatentPlanPolicy(mod, n_envs=3, plan_duration=16)
    pol.reset()
    for t in range(3):
        a = pol.step(obs[:, t], goal, noise={"rand_a": tape[1 + 2 * t][1], "rand_b": tape[2 + 2 * t][1]})
        if t == 0:
            assert _rel(pol.plan, z["plan"]) < 1e-4
        assert a.shape == (3, 8) and _rel(a, z["actions"][t][:, 0]) < 1e-3, (t, _rel(a, z["actions"][t][:, 0]))
    assert _rel(torch.stack(list(pol.hidden)), z["hidden"]) < 1e-4
    mod.action_decoder.clear_hidden_state()
    a = mod.action_decoder.act(latent_plan=torch.from_numpy(z["plan"]).to(DEV), perceptual_emb=obs[:, 0].unsqueeze(1),
                               noise=(tape[1][1], tape[2][1]))
    assert _rel(a[:, 0], z["actions"][0][:, 0]) < 1e-3
    # the critics are callable, and CEMOptimizer takes them
    for name in ("q1", "q2", "target_q1", "target_q2"):
        q = getattr(mod, name)(og, plan)
        assert q.shape == (3, 1) and bool(torch.isfinite(q).all())
    cem = CEMOptimizer(q1=mod.q1, q2=mod.q2, action_dim=16)
    eps = torch.randn(2, cem.num_iterations, cem.batch_size, 16, generator=torch.Generator().manual_seed(1))
    refined = cem.get_action(og[:2], initial_mean=plan[:2], noise={"eps": eps})
    assert refined.shape == (2, 16) and bool((refined.abs() <= 1).all())
    sd = {k: v.detach().double().cpu() for k, v in mod.state_dict().items() if k.startswith("q1.Q.")}

    def q_fn(emb, actions):
        x = torch.cat([emb.expand(actions.shape[0], -1), actions], dim=-1)
        i = 0
        while f"q1.Q.fc_layers.{i}.weight" in sd:
            x = torch.nn.functional.silu(x @ sd[f"q1.Q.fc_layers.{i}.weight"].T + sd[f"q1.Q.fc_layers.{i}.bias"])
            i += 1
        return x @ sd["q1.Q.out.weight"].T + sd["q1.Q.out.bias"]

    for r in range(2):
        best, trace = cem_restatement(q_fn, og[r].double().cpu(), plan[r].double().cpu(), eps[r].double(),
                                      n_elite=n_elite_of(cem.batch_size, cem.elite_fraction), min_std=cem.min_std,
                                      max_std=cem.max_std, alpha=cem.alpha)
        q_best = max(float(q[e[0]]) for q, e in zip(trace["q"], trace["elite"]))
        got = float(mod.q1(og[r], refined[r])[0, 0])
        assert abs(got - q_best) <= 1e-4 * max(abs(q_best), 1.0), (r, got, q_best)
    pol_cem = LatentPlanPolicy(mod, n_envs=3, plan_duration=16, use_cem=True)
    a = pol_cem.step(obs[:, 0], goal)
    assert a.shape == (3, 8) and bool(torch.isfinite(a).all()) and bool((pol_cem.plan.abs() <= 1).all())


# ------------------------------------------------------------------------------------------ episodes
def test_rollout_episodes_four_at_once_equal_four_alone():
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy, rollout_episodes

    torch.manual_seed(2)
    lmp = K.build(K.playlmp_d4rl_cfg(latent=16, T=8, device=DEV, dropout_p=0.0))
    lmp.eval()
    lengths = [5, 9, 9, 12]
    envs = lambda: [V.LinearEnv(seed=40 + i, length=n) for i, n in enumerate(lengths)]  # noqa: E731
    g = torch.Generator().manual_seed(8)
    draws = [dict(plan_eps=torch.randn(4, 16, generator=g), rand_a=torch.rand(4, 8, 10, generator=g), rand_b=torch.rand(4, 8, generator=g))
             for _ in range(max(lengths))]
    pol = LatentPlanPolicy(lmp, n_envs=4, plan_duration=4)
    infos = rollout_episodes(pol, envs(), noise=lambda t: draws[t])
    assert [i["episode_length"] for i in infos] == lengths
    assert all(set(i) == {"episode_length", "episode_return", "success"} for i in infos)
    for r, env in enumerate(envs()):
        one = rollout_episodes(LatentPlanPolicy(lmp, n_envs=1, plan_duration=4), [env],
                               noise=lambda t, r=r: {k: v[r: r + 1] for k, v in draws[t].items()})[0]
        assert one["episode_length"] == infos[r]["episode_length"]
        assert one["episode_return"] == infos[r]["episode_return"], (r, one["episode_return"], infos[r]["episode_return"])
    capped = rollout_episodes(pol, envs(), max_steps=3, noise=lambda t: draws[t])
    assert [i["episode_length"] for i in capped] == [3, 3, 3, 3]



# ------------------------------------------------------------------------------------------ routing
class _CallLog:
    """The entry points ActionDecoderLogistic calls, in order (a wrapper around the module's `call`)."""

    def __init__(self, monkeypatch):
        import tacorl_amd.networks.action_decoder as M

        self.names, real = [], M.call
        monkeypatch.setattr(M, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


def test_step_rows_routes_by_row_count(monkeypatch):
    """Up to ActionDecoderLogistic.ROWS_KERNEL_MAX_R rows a step is one tacorl_rows_linear2_fwd per RNN layer and one for the
    heads; above it, the kernels `act` is made of (profiles/vec_rollout.md: from the second row group on the rows kernel is the
    slower one).  Asserted from the entry points the step called."""
    from tacorl_amd.networks.action_decoder import ActionDecoderLogistic

    pb = V.decoder_problem(72)
    ad = _decoder(pb)
    M = ActionDecoderLogistic.ROWS_KERNEL_MAX_R
    assert 1 <= M < 64 and M % G() == 0  # whole row groups: a part-filled group costs the rows kernel a full weight pass
    log = _CallLog(monkeypatch)
    for R, route in ((1, "rows"), (M, "rows"), (M + 1, "composed"), (64, "composed")):
        assert ad.rows_route(R) == route
        st = ad.new_rows_state(R)
        plan, emb = torch.zeros(R, pb["P"], device=DEV), torch.zeros(R, pb["E"], device=DEV)
        del log.names[:]
        a = ad.step_rows(st, plan, emb, [True] * R)
        assert a.shape == (R, 7) and bool(torch.isfinite(a).all())
        n_rows, n_gemm = log.names.count("tacorl_rows_linear2_fwd"), log.names.count("tacorl_linear_add_fwd")
        assert (n_rows, n_gemm) == ((pb["L"] + 1, 0) if route == "rows" else (0, 2 * pb["L"] + 1)), (R, log.names)
        assert log.names[0] == "tacorl_build_ad_input" and log.names[-1] == "tacorl_logistic_mixture_sample"


@pytest.mark.parametrize("H", [2048, 72])
def test_step_rows_composed_route_against_the_rows_kernel(H):
    """Both routes of step_rows on one problem (the composed one forced at R = 3): every layer of the composed route inside its
    a-priori bound on its own operands, the two routes' hidden states and heads inside vec_rollout_util.cross_path_bounds,
    actions equal at 1e-4 relative (no case of this seed is near a tie: tests/test_vec_policy_cpu.py), and a restarted row
    whose buffers hold NaN comes out finite on both (row 1 at step 2)."""
    pb = V.decoder_problem(H)
    R, L, NH = pb["R"], pb["L"], 3 * pb["Da"] * pb["K"] + 2
    ad = _decoder(pb)
    st_k, st_c = ad.new_rows_state(R), ad.new_rows_state(R)
    plan = pb["plan"].to(DEV)
    h_k = [torch.zeros(R, H, dtype=torch.float64) for _ in range(L)]
    h_c = [torch.zeros(R, H, dtype=torch.float64) for _ in range(L)]
    for t in range(pb["steps"]):
        emb, noise = pb["emb"][t].to(DEV), (pb["ra"][t].to(DEV), pb["rb"][t].to(DEV))
        if t == 2:
            for st in (st_k, st_c):
                for h in st.hidden:
                    h[1] = float("nan")
        ad.ROWS_KERNEL_MAX_R = 64
        a_k = ad.step_rows(st_k, plan, emb, pb["restart"][t], noise=noise).clone()
        ad.ROWS_KERNEL_MAX_R = 0
        try:
            a_c = ad.step_rows(st_c, plan, emb, pb["restart"][t], noise=noise).clone()
        finally:
            del ad.ROWS_KERNEL_MAX_R
        new_k, new_c = [h.double().cpu() for h in st_k.hidden], [h.double().cpu() for h in st_c.hidden]
        ref_k, ref_c = V.decoder_step64(pb, t, h_k, own_h=new_k), V.decoder_step64(pb, t, h_c, own_h=new_c)
        lb, hb = V.cross_path_bounds(pb, t, ref_k, ref_c, h_k, h_c, new_k, new_c)
        for l in range(L):
            assert bool(((new_c[l] - ref_c[4][l]).abs() <= ref_c[5][l]).all()), (t, l)
            assert bool(((new_k[l] - new_c[l]).abs() <= lb[l]).all()), (t, l)
        assert bool(((st_k.heads[:, :NH].double().cpu() - st_c.heads[:, :NH].double().cpu()).abs() <= hb).all()), t
        assert bool(torch.isfinite(a_k).all()) and bool(torch.isfinite(a_c).all())
        assert torch.equal(a_k[:, -1], a_c[:, -1])
        assert bool(((a_k[:, :-1] - a_c[:, :-1]).abs() <= 1e-4 * a_c[:, :-1].abs()).all()), t
        h_k, h_c = new_k, new_c
