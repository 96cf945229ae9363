"""CQL_Offline with goal cameras that differ from the observation cameras (config/experiment/cql_gripper_real_world.yaml:
obs = [rgb_static, rgb_gripper], goal = [rgb_static]) on the GPU: against the unmodified reference's fixture
(tests/golden/cql_goalcams.npz) and the CPU restatement, at the bounds of tests/test_step_gpu.py for the same arithmetic."""
import copy
import os
import sys

import pytest
import torch

from tacorl_amd import synth
from tests import goalcams_util as U
from tests.golden_util import Golden, check_stats, gradient_floor, resync_oracle
from tests.proc_util import free_port, run_group
from tests.test_step_gpu import (GRAD_RTOL, PARAM_ATOL, RTOL, _bf16_compare, _snap, _with_bf16_sensitivity, check_logs,
                                 compare_with_oracle_grads, to_dev)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    g = Golden(U.NAME)
    return g, g.cfg["obs_cams"], g.cfg["goal_cams"]


def _got(mod):
    return {k.split("/", 1)[1]: v for k, v in mod.logged.items()}


def test_reference_parity_f32():
    """The body of test_step_gpu.test_cql_offline_step on the asymmetric fixture: state-dict keys and shapes, logged scalars
    (RTOL) on both steps, gradients against the restatement (GRAD_RTOL, gradient floor), the golden's gradient fingerprints
    at step 0, parameters after each step (RTOL / PARAM_ATOL)."""
    from oracle import tacorl_oracle as O

    g, obs_c, goal_c = _fixture()
    mod = U.build(obs_c, goal_c)
    sd = mod.state_dict()
    assert sorted(sd) == sorted(g.names)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(zip(g.names, (tuple(s) for s in g.shapes)))
    mod.load_state_dict(g.params())
    mod.current_epoch = g.cfg["epoch"]
    spec = U.spec_of(obs_c, goal_c)
    P = O.require_grad_(g.params())
    opts = O.make_opts(P, spec)
    for step in range(g.cfg["steps"]):
        batch, noise = g.batch(step), g.noise(step)
        if step:
            resync_oracle(mod, P, opts)
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), 0, noise=to_dev(noise, mod.device))
        torch.cuda.synchronize()
        got = _got(mod)
        before, opts0 = _snap(P), copy.deepcopy(opts)
        _, ograds = O.cql_step(P, opts, spec, batch, noise, g.cfg["epoch"])
        floor = gradient_floor(lambda Pp: O.cql_step(Pp, copy.deepcopy(opts0), spec, batch, noise, g.cfg["epoch"])[1], before, ograds)
        bad = check_logs(got, g.logged(step))
        bad += compare_with_oracle_grads(mod, ograds, GRAD_RTOL, floor)
        if step == 0:
            bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=GRAD_RTOL, what="golden grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


@pytest.mark.parametrize("obs_c,goal_c", [(["rgb_gripper", "rgb_static"], ["rgb_static"]),
                                          (["rgb_static", "rgb_gripper"], ["rgb_gripper"]),
                                          (["rgb_gripper"], ["rgb_static"])], ids=["obs-gs-goal-s", "obs-sg-goal-g", "disjoint"])
def test_column_order_and_disjoint_roles_f32(obs_c, goal_c):
    """One step against the restatement alone (synth parameters and batch, the two geometries differ): the observation
    cameras in an order that is not the sorted one, the goal camera in the second observation column, and disjoint roles -
    there the goal-only camera's encoders get the goal gradient in actor, q1 and q2, and the targets' copies follow Polyak."""
    from oracle import tacorl_oracle as O

    seed, epoch = 57, 5
    mod = U.build(obs_c, goal_c)
    params = U.synth_params(mod, seed)
    mod.load_state_dict(params)
    mod.current_epoch = epoch
    spec = U.spec_of(obs_c, goal_c)
    P = O.require_grad_({k: v.clone() for k, v in params.items()})
    opts = O.make_opts(P, spec)
    batch, noise = synth.make_transition_batch(seed * 100, 3, U.GEOM), U.synth_noise(seed, 3)
    mod.logged = {}
    mod.training_step(to_dev(batch, mod.device), 0, noise=to_dev(noise, mod.device))
    torch.cuda.synchronize()
    before, opts0 = _snap(P), copy.deepcopy(opts)
    ologs, ograds = O.cql_step(P, opts, spec, batch, noise, epoch)
    floor = gradient_floor(lambda Pp: O.cql_step(Pp, copy.deepcopy(opts0), spec, batch, noise, epoch)[1], before, ograds)
    bad = check_logs(_got(mod), ologs)
    bad += compare_with_oracle_grads(mod, ograds, GRAD_RTOL, floor)
    after = {k: synth.tensor_stats(v) for k, v in P.items()}
    sd = mod.state_dict()
    bad += check_stats(sd, after, rtol=RTOL, atol=PARAM_ATOL, what="param ")
    assert not bad, "\n".join(bad[:25])
    if not set(obs_c) & set(goal_c):
        grads = mod.named_gradients()
        for net in ("actor", "q1", "q2"):
            gk = [k for k in grads if k.startswith(f"{net}.encoder.networks.rgb_static.")]
            assert gk and all(float(grads[k].norm()) > 0 and float(ograds[k].norm()) > 0 for k in gk), net
        for t in ("target_q1", "target_q2"):
            tk = [k for k in sd if k.startswith(f"{t}.encoder.networks.rgb_static.")]
            assert tk and all(not torch.equal(sd[k].cpu(), params[k]) for k in tk), t


def _bf16_steps(mod, params, spec, batches, noises, epoch):
    from oracle import tacorl_oracle as O

    mod.load_state_dict(params)
    mod.current_epoch = epoch
    P = O.require_grad_({k: v.clone() for k, v in params.items()})
    opts = O.make_opts(P, spec)
    bad = []
    for step, (batch, noise) in enumerate(zip(batches, noises)):
        if step:
            resync_oracle(mod, P, opts)
        before = _snap(P)
        mod.logged = {}
        mod.training_step(to_dev(batch, mod.device), 0, noise=to_dev(noise, mod.device))
        torch.cuda.synchronize()
        opts0 = copy.deepcopy(opts)
        with O.operand_rounding(torch.bfloat16):
            ologs, ograds = O.cql_step(P, opts, spec, batch, noise, epoch)
            floor = gradient_floor(lambda Pp: O.cql_step(Pp, copy.deepcopy(opts0), spec, batch, noise, epoch)[1], before, ograds)
        floor = _with_bf16_sensitivity(floor, ograds, O.cql_step(_snap(before), copy.deepcopy(opts0), spec, batch, noise, epoch)[1])
        bad += _bf16_compare(mod, _got(mod), ologs, ograds, before, P, step, floor=floor)
    return bad


def _assert_fast_path(mod):
    """What the step records about the path it took.  The library binding keeps no launch counter or call trace, so the
    fused entry points are pinned through the decisions the engine itself branches on and caches while the step runs:
    `_fused_ok` / `_fused_bwd_ok` per camera (fused encoder forward, LDS-resident conv backward), `_gather_cache` (written
    by the forward assembly: the gather-fed first layer of the goal encoders and the policy head; the Q heads' action block
    has a pitch of 7 floats, which the gathered forward does not take - the same for the symmetric CQL step) and
    `_lean_cache` (a site is lean only when its forward, input-gradient chain and weight gradients are all the fused
    launches).  The Q site's fused forward has no record of its own: its predicate is queried with the step's widths."""
    from tacorl_amd import ops

    e = mod.engine
    assert e.compute == 1 and e.use_fused
    for c in e.enc_cams:
        assert e._fused_ok(c) and e._fused_bwd_ok(c), c
    assert sorted(c for cs in e._fused_groups() for c in cs) == sorted(e.enc_cams)
    B = e.B
    assert e._gather_cache == {("genc", B): True, ("pi", B): True, ("q", B): False}, e._gather_cache
    assert e._lean_cache == {"genc": True, "pi": True, "q": True}, e._lean_cache
    qd = e.q1.head_dims
    assert qd[0] == e.E + 7 and e.ldq == 104
    assert ops.L.lib().tacorl_mlp_fwd_fused_supported(6, len(qd) - 1, ops.int_array(qd), e.ldq)
    for tag, params, M, dims in e._mlp_bwd_sites():
        ldo, ldd = {"q": (1, e.ldq), "qpi": (1, e.ldq), "pi": (e.HD, e.lds), "genc": (e.lds, e.G)}[tag]
        assert ops.mlp_bwd_fused_ok(len(params), dims, ldo, ldd, e.compute), tag


def test_bf16_fast_path_vs_rounded_oracle():
    """test_step_gpu.test_cql_step_bf16_vs_rounded_oracle on the fixture's configuration, and the step took the fused path."""
    g, obs_c, goal_c = _fixture()
    mod = U.build(obs_c, goal_c, "bf16")
    steps = range(g.cfg["steps"])
    bad = _bf16_steps(mod, g.params(), U.spec_of(obs_c, goal_c), [g.batch(s) for s in steps], [g.noise(s) for s in steps],
                      g.cfg["epoch"])
    _assert_fast_path(mod)
    assert not bad, "\n".join(bad[:30])


def test_bf16_fast_path_experiment_geometry():
    """The experiment's geometry - rgb_static 150 x 200 (a ring-kernel camera) beside rgb_gripper 84 x 84 - at B = 2, one step."""
    obs_c, goal_c = ["rgb_static", "rgb_gripper"], ["rgb_static"]
    geom = {"rgb_static": (150, 200), "rgb_gripper": (84, 84)}
    seed = 59
    mod = U.build(obs_c, goal_c, "bf16")
    bad = _bf16_steps(mod, U.synth_params(mod, seed), U.spec_of(obs_c, goal_c), [synth.make_transition_batch(seed * 100, 2, geom)],
                      [U.synth_noise(seed, 2)], 5)
    _assert_fast_path(mod)
    e = mod.engine
    assert e.X3["rgb_static"].shape == (6, 150, 200, 3) and e.X3["rgb_gripper"].shape == (4, 84, 84, 3)
    assert not bad, "\n".join(bad[:30])


def _same(ma, mb):
    assert ma.logged == mb.logged and ma.logged, (ma.logged, mb.logged)
    sa, sb = ma.state_dict(), mb.state_dict()
    assert sorted(sa) == sorted(sb)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_unused_images_are_not_needed(compute):
    """The wrist camera is no goal camera: with its images dropped from both `goal` dicts the step is bit-identical."""
    g, obs_c, goal_c = _fixture()
    batch, noise = g.batch(0), g.noise(0)
    lean = copy.deepcopy(batch)
    for side in ("observations", "next_observations"):
        lean[side]["goal"] = {c: v for c, v in lean[side]["goal"].items() if c in goal_c}
        assert sorted(lean[side]["goal"]) == ["rgb_static"]
    mods = []
    for b in (batch, lean):
        m = U.build(obs_c, goal_c, compute)
        m.load_state_dict(g.params())
        m.current_epoch = g.cfg["epoch"]
        m.logged = {}
        m.training_step(to_dev(b, m.device), 0, noise=to_dev(noise, m.device))
        mods.append(m)
    torch.cuda.synchronize()
    _same(*mods)


def test_uint8_frames_equal_host_normalised_fp32():
    """The dataset's uint8 HWC frames (only the images a role uses) against the host-transformed fp32 CHW route."""
    g, obs_c, goal_c = _fixture()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(13)
    B = 3
    u8 = lambda c: torch.randint(0, 256, (B, *U.GEOM[c], 3), device=dev, dtype=torch.uint8, generator=gen)  # noqa: E731
    o8, x8, g8 = {c: u8(c) for c in obs_c}, {c: u8(c) for c in obs_c}, {c: u8(c) for c in goal_c}
    # torchvision ToTensor + Normalize(0.5, 0.5) on the CPU, as the dataloader workers run them (test_fullsize_gpu.py)
    chw = lambda x: ((x.cpu().float().div(255) - 0.5) / 0.5).to(dev).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    base = to_dev(g.batch(0), dev)
    mkb = lambda f: dict(base, observations={"observation": {c: f(v) for c, v in o8.items()}, "goal": {c: f(v) for c, v in g8.items()}},  # noqa: E731
                         next_observations={"observation": {c: f(v) for c, v in x8.items()}, "goal": {c: f(v) for c, v in g8.items()}})
    mods = []
    for b in (mkb(chw), mkb(lambda x: x)):
        m = U.build(obs_c, goal_c, "bf16")
        m.load_state_dict(g.params())
        m.current_epoch = g.cfg["epoch"]
        m.logged = {}
        m.training_step(b, 0, noise=to_dev(g.noise(0), dev))
        mods.append(m)
    torch.cuda.synchronize()
    for c in obs_c:
        assert torch.equal(mods[0].engine.X3[c], mods[1].engine.X3[c]), c
    _same(*mods)


def test_hipgraph_equals_eager():
    """enable_graph() (warm-up + capture, then a replay) against the eager module on the same batches and noise, and both
    against the reference's fixture - the standard of test_step_gpu.test_tacorl_step_hipgraph."""
    g, obs_c, goal_c = _fixture()
    mods = [U.build(obs_c, goal_c), U.build(obs_c, goal_c)]
    for m in mods:
        m.load_state_dict(g.params())
        m.current_epoch = g.cfg["epoch"]
    mods[0].enable_graph()
    for step in (0, 1, 1):  # capture, capture-or-replay, replay
        for m in mods:
            m.logged = {}
            m.training_step(to_dev(g.batch(step), m.device), 0, noise=to_dev(g.noise(step), m.device))
        torch.cuda.synchronize()
        a, b = mods[0].logged, mods[1].logged
        assert a.keys() == b.keys()
        bad = [f"{k}: graph {a[k]:.9g} eager {b[k]:.9g}" for k in a if abs(a[k] - b[k]) > 1e-6 * max(abs(b[k]), 1e-3)]
        assert not bad, "\n".join(bad)
    sa, sb = mods[0].state_dict(), mods[1].state_dict()
    worst = max(((sa[k].double() - sb[k].double()).norm() / sb[k].double().norm()).item() for k in sa if sb[k].norm() > 0)
    assert worst < 1e-6, worst
    assert len(mods[0]._graphs) == 1 and torch.isfinite(mods[0].engine.logs).all()
    # the first two steps are the fixture's: the graph-mode module is where the reference is
    m = U.build(obs_c, goal_c)
    m.load_state_dict(g.params())
    m.current_epoch = g.cfg["epoch"]
    m.enable_graph()
    for step in range(g.cfg["steps"]):
        m.logged = {}
        m.training_step(to_dev(g.batch(step), m.device), 0, noise=to_dev(g.noise(step), m.device))
        torch.cuda.synchronize()
        bad = check_logs(_got(m), g.logged(step))
        bad += check_stats(m.state_dict(), g.stats(step, "param"), rtol=RTOL, atol=PARAM_ATOL, what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


def test_validation_step_logs_and_moves_nothing():
    g, obs_c, goal_c = _fixture()
    mod = U.build(obs_c, goal_c)
    mod.load_state_dict(g.params())
    mod.current_epoch = g.cfg["epoch"]
    mod.eval()
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    mod.logged = {}
    mod.validation_step(to_dev(g.batch(0), mod.device), 0, noise=to_dev(g.noise(0), mod.device))
    torch.cuda.synchronize()
    exp = g.logged(0)
    assert sorted(mod.logged) == sorted("validation/" + k for k in exp), sorted(mod.logged)
    got = _got(mod)
    # the critics' forward does not depend on the alpha step, which is the one thing a validation step leaves out
    same = ("q1_data", "q2_data", "q1_random", "q2_random", "q1_policy", "q2_policy", "alpha_loss")
    assert not check_logs({k: got[k] for k in same}, {k: exp[k] for k in same})
    assert all(torch.isfinite(torch.tensor(v)) for v in got.values())
    after = mod.state_dict()
    assert not [k for k, v in before.items() if not torch.equal(v, after[k])]


def test_one_rank_rccl_collectives_equal_the_collective_free_step():
    """TACORL_FORCE_COLLECTIVES=1, backend nccl (RCCL), one rank, in a fresh child process (tests/goalcams_rccl_script.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    out = run_group([sys.executable, os.path.join(ROOT, "tests", "goalcams_rccl_script.py")], env, ROOT, timeout=240)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "librccl" in out.stdout


def test_rollout_surfaces_and_cem():
    """actor.get_actions / q1(obs, a) / get_emb_representation on the dict observation against the restatement's _emb /
    policy / qnet at 1e-4, and CEMOptimizer.get_action with injected draws against cem_restatement at the bounds of
    tests/test_cem_gpu.py (elite order, Q, mean, std and the action at 1e-4, the gripper exact)."""
    from tacorl_amd.modules.cem import CEMOptimizer
    from tests.cem_util import rel, rel_gaps, same_elite_order

    obs_c, goal_c = ["rgb_static", "rgb_gripper"], ["rgb_static"]
    mod = U.build(obs_c, goal_c)
    P = U.surface_params({k: tuple(v.shape) for k, v in mod.state_dict().items() if v.dtype == torch.float32})
    mod.load_state_dict(P)
    mod.eval()
    obs = synth.make_transition_batch(U.SURF_SEED * 100, 1, U.GEOM)["observations"]
    emb, a_det, eps, act_ref, tr_ref = U.surface_restatement(P, obs, U.spec_of(obs_c, goal_c))
    # (the yardstick's own condition, as for the CEM fixtures: the selection boundary and the best candidate stay apart)
    assert min(gp for q in tr_ref["q"] for gp in rel_gaps(q.numpy(), U.CEM_ELITE)) >= U.CEM_GAP
    dobs = to_dev(obs, mod.device)
    for name, box in (("actor", mod.actor), ("q1", mod.q1), ("q2", mod.q2)):
        s = box.get_emb_representation(dobs)
        assert s.shape == (1, 96) and rel(s, emb[name]) < 1e-4, (name, rel(s, emb[name]))
    assert mod.q1.get_emb_obs_representation(dobs).shape == (1, 64)
    a, lp = mod.actor.get_actions(dobs, deterministic=True)
    assert a.shape == (1, 7) and rel(a, a_det) < 1e-4 and float(a[0, -1]) == float(a_det[0, -1]) and float(lp.abs().max()) == 0.0
    from oracle import tacorl_oracle as O

    pop = tr_ref["pop"][0].float()
    with torch.no_grad():
        q_ref = O.qnet(P, "q1.critic.Q.", emb["q1"].expand(pop.shape[0], -1), pop)
    q = mod.q1(dobs, pop.to(mod.device))
    assert q.shape == (U.CEM_N, 1) and rel(q, q_ref) < 1e-4, rel(q, q_ref)
    cem = CEMOptimizer(q1=mod.q1, q2=mod.q2, batch_size=U.CEM_N, num_iterations=U.CEM_ITERS, elite_fraction=U.CEM_ELITE / U.CEM_N,
                       action_dim=7, discrete_gripper=True, twin_min=True)
    assert cem.n_elite == U.CEM_ELITE
    act, tr = cem.get_action(dobs, initial_mean=a_det.float(), noise={"eps": eps}, return_trace=True)
    assert act.shape == (1, 7)
    for it in range(U.CEM_ITERS):
        assert same_elite_order(tr["elite"][0, it].cpu(), tr_ref["elite"][it], tr_ref["q"][it], U.CEM_ORDER_GAP), it
        for k in ("pop", "q", "mean", "std"):
            assert rel(tr[k][0, it], tr_ref[k][it]) < 1e-4, (it, k, rel(tr[k][0, it], tr_ref[k][it]))
    assert rel(act[0], act_ref) < 1e-4 and float(act[0, -1]) == float(act_ref[-1]) and abs(float(act[0, -1])) == 1.0
