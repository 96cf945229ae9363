"""CEM plan refinement and the critic rollout surface on the GPU, against traces recorded from the unmodified reference
CEMOptimizer (tests/golden/cem_*.npz; tools/gen_cem_golden.py) with the modules built the way tests/test_rollout_gpu.py
builds them (TACORL from a reference PlayLMP run directory)."""
import pytest
import torch

from tests import cfg_util as C
from tests.cem_util import CemGolden, q_fn_of, q_head, rel, same_elite_order

pytestmark = pytest.mark.gpu

CASES = {"cem_cql": ("n64_actor", "n64_actor_twin", "n64_zero", "n64_zero_twin", "n256_actor", "n256_zero_twin"),
         "cem_tacorl": ("n64_actor_twin", "n64_zero", "n256_actor", "n256_zero_twin")}
FILES = tuple(CASES)
FILE_CASES = [(f, c) for f in FILES for c in CASES[f]]
_mods = {}


def _module(name, compute, tmp_path_factory):
    """One module per (fixture, compute mode) for the whole file: building TACORL goes through a run directory on disk."""
    if (name, compute) in _mods:
        return _mods[(name, compute)]
    g = CemGolden(name)
    params = g.params()
    if name == "cem_tacorl":
        from tacorl_amd.modules.tacorl.tacorl import TACORL

        d = tmp_path_factory.mktemp("lmp_run")
        C.write_reference_run_dir(str(d), C.lmp_state_dict_from_tacorl(params))
        strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
        mod = TACORL(play_lmp_dir=str(d), compute_dtype=compute, image_dtype="f32",
                     **strip(C.tacorl_cfg(device="cuda:0", finetune_action_decoder=False)))
        missing, unexpected = mod.load_state_dict(params, strict=False)
        assert not unexpected, unexpected
    else:
        from tacorl_amd.lightning import instantiate

        mod = instantiate(C.cql_cfg(device="cuda:0", compute_dtype=compute, image_dtype="f32"))
        mod.load_state_dict(params)
    mod.eval()
    _mods[(name, compute)] = (g, mod)
    return g, mod


def _cem(g, mod, c, **kw):
    from tacorl_amd.modules.cem import CEMOptimizer

    hp = c["hp"]
    return CEMOptimizer(q1=mod.q1, q2=mod.q2, batch_size=hp["batch_size"], num_iterations=hp["num_iterations"],
                        elite_fraction=hp["elite_fraction"], min_std=hp["min_std"], max_std=hp["max_std"], alpha=hp["alpha"],
                        action_dim=mod.actor.action_dim, discrete_gripper=mod.actor.discrete_gripper,
                        twin_min=hp["twin_min"], **kw)


def _to_dev(obs, dev):
    return {k: {c: v.to(dev) for c, v in d.items()} for k, d in obs.items()}


@pytest.mark.parametrize("name", FILES)
def test_critic_surface_against_golden_q(name, tmp_path_factory):
    """module.q1(obs, a) = the as-written traces' Q, min(q1, q2)(obs, a) = the twin traces' Q, f32 at 1e-4 relative; image
    and embedding input, batched and unbatched; q2 on its own against the fp64 Q head on the recorded q2 embedding."""
    g, mod = _module(name, "f32", tmp_path_factory)
    dev = mod.device
    aw, tw = g.case("n256_actor"), g.case("n256_zero_twin")
    obs_b, obs_u = _to_dev(g.obs(True), dev), _to_dev(g.obs(False), dev)
    for obs in (obs_b, obs_u):
        q1 = mod.q1(obs, aw["pop"][0].to(dev))
        assert q1.shape == (256, 1)
        e = rel(q1.reshape(-1), aw["q"][0])
        print(f"{name} q1 images: rel {e:.3g}")
        assert e < 1e-4
        a = tw["pop"][1].to(dev)
        qm = torch.minimum(mod.q1(obs, a), mod.q2(obs, a))
        e = rel(qm.reshape(-1), tw["q"][1])
        print(f"{name} min(q1, q2) images: rel {e:.3g}")
        assert e < 1e-4
    # embeddings: the critic's own, and the recorded ones
    s1, s2 = mod.q1.get_emb_representation(obs_b), mod.q2.get_emb_representation(obs_u)
    assert s1.shape == s2.shape == (1, g.emb("q1").numel()) and not torch.equal(s1, s2)
    assert rel(s1[0], g.emb("q1")) < 1e-4 and rel(s2[0], g.emb("q2")) < 1e-4
    so = mod.q1.get_emb_obs_representation(obs_b)
    assert so.shape == (1, s1.shape[1] // 2) and torch.equal(so, s1[:, : so.shape[1]])
    a = aw["pop"][2].to(dev)
    for emb in (s1, s1[0], g.emb("q1").float()):
        assert rel(mod.q1(emb, a).reshape(-1), aw["q"][2]) < 1e-4
    one = mod.q1(s1[0], a[3])  # unbatched embedding, unbatched action
    assert one.shape == (1, 1) and rel(one.reshape(-1), aw["q"][2][3:4]) < 1e-4
    q2_ref = q_head(g.params(), "q2", torch.float64)(g.emb("q2"), a.cpu())
    for which in ("q2", "target_q2"):  # (the fixture's target critics carry their own parameters)
        got = getattr(mod, which)(obs_b, a)
        assert got.shape == (256, 1) and torch.isfinite(got).all()
    assert rel(mod.q2(obs_b, a).reshape(-1), q2_ref) < 1e-4


@pytest.mark.parametrize("name,cname", FILE_CASES)
def test_cem_f32_against_reference_trace(name, cname, tmp_path_factory):
    """get_action with the recorded draws, f32, on the unbatched image observation the reference ran on: per iteration the
    reference's elite indices in the reference's order (descending Q), and Q, mean, std within 1e-4 relative; the returned
    action within 1e-4 with the gripper exact.  The fixtures keep the selection boundary and the top >= 1e-3 max|Q| apart;
    the order inside is compared position by position wherever the reference's neighbouring elites are >= 1e-4 max|Q| apart
    (the tolerance of this comparison - closer ones may swap and are compared as a set, cem_util.same_elite_order)."""
    g, mod = _module(name, "f32", tmp_path_factory)
    c = g.case(cname)
    hp = c["hp"]
    cem = _cem(g, mod, c)
    act, tr = cem.get_action(_to_dev(g.obs(False), mod.device), initial_mean=c["mean0"].float() if c["mean0"] is not None else None,
                             noise={"eps": c["eps"]}, return_trace=True)
    assert act.shape == (hp["action_dim"],)
    exact = 0
    for it in range(hp["num_iterations"]):
        el = tr["elite"][0, it].cpu()
        assert same_elite_order(el, c["elite"][it], c["q"][it], g.cfg["order_gap"]), (it, el, c["elite"][it])
        exact += int(torch.equal(el, c["elite"][it]))
        for k in ("pop", "q", "mean", "std"):
            e = rel(tr[k][0, it], c[k][it])
            print(f"{name}/{cname} iteration {it} {k}: rel {e:.3g}")
            assert e < 1e-4, (it, k, e)
    print(f"{name}/{cname}: elite order identical in {exact} of {hp['num_iterations']} iterations")
    e = rel(act, c["action"])
    print(f"{name}/{cname} action: rel {e:.3g}")
    assert e < 1e-4
    if hp["discrete_gripper"]:
        assert float(act[-1]) == float(c["action"][-1]) and abs(float(act[-1])) == 1.0


@pytest.mark.parametrize("name,cname", [("cem_cql", "n64_zero_twin"), ("cem_cql", "n256_actor"),
                                        ("cem_tacorl", "n64_actor_twin"), ("cem_tacorl", "n256_actor")])
def test_cem_bf16_two_halves(name, cname, tmp_path_factory):
    """bf16 cannot be required to select the reference's elites, so: (1) the trace's Q values on the trace's own populations
    agree with the Q head evaluated with bf16-rounded operands within 3e-2 relative (the bound tests/test_rollout_gpu.py holds
    bf16 actor outputs to); (2) given the device's own fp32 Q values, an fp64 recomputation of selection, refit and best
    action gives the same elite indices exactly and pop / mean / std / action within 1e-6."""
    g, mod = _module(name, "bf16", tmp_path_factory)
    c = g.case(cname)
    hp = c["hp"]
    cem = _cem(g, mod, c)
    # a tensor observation IS the embedding, for both critics: the arithmetic is under test here, not the encoders
    emb = g.emb("q1").float().reshape(1, -1)
    mean0 = c["mean0"].float() if c["mean0"] is not None else None
    act, tr = cem.get_action(emb, initial_mean=mean0, noise={"eps": c["eps"]}, return_trace=True)
    act = act[0].cpu()
    tr = {k: v[0].cpu() for k, v in tr.items()}
    q_bf = q_fn_of(g.params(), hp["twin_min"], torch.float64, bf16_operands=True)
    mean = mean0.double() if mean0 is not None else torch.zeros(hp["action_dim"], dtype=torch.float64)
    std = torch.full_like(mean, hp["max_std"])
    best_q, best_a, ne = -float("inf"), None, c["n_elite"]
    for it in range(hp["num_iterations"]):
        e = rel(tr["q"][it], q_bf((emb[0], emb[0]), tr["pop"][it].double()))
        print(f"{name}/{cname} iteration {it} bf16 q: rel {e:.3g}")
        assert e < 3e-2, (it, e)
        pop = (mean + c["eps"][it].double() * std).clamp(-1.0, 1.0)
        if hp["discrete_gripper"]:
            pop[:, -1] = torch.where(pop[:, -1] >= 0, 1.0, -1.0).double()
        assert rel(tr["pop"][it], pop) < 1e-6
        if hp["discrete_gripper"]:
            assert torch.equal(tr["pop"][it][:, -1].double(), pop[:, -1])
        q = tr["q"][it].double()
        el = torch.argsort(q, descending=True, stable=True)[:ne]
        assert torch.equal(tr["elite"][it].long(), el), (it, tr["elite"][it], el)
        elites = tr["pop"][it].double()[el]
        m = hp["alpha"] * tr["mean"][it - 1].double() if it else hp["alpha"] * mean
        s = hp["alpha"] * tr["std"][it - 1].double() if it else hp["alpha"] * std
        mean_n = m + (1 - hp["alpha"]) * elites.mean(0)
        std_n = (s + (1 - hp["alpha"]) * elites.std(0)).clamp(hp["min_std"], hp["max_std"])
        assert rel(tr["mean"][it], mean_n) < 1e-6 and rel(tr["std"][it], std_n) < 1e-6, (it, rel(tr["mean"][it], mean_n))
        if float(q[el[0]]) > best_q:
            best_q, best_a = float(q[el[0]]), tr["pop"][it][el[0]]
        mean, std = tr["mean"][it].double(), tr["std"][it].double()  # the device's own state starts the next iteration
    assert rel(act, best_a) < 1e-6


def test_rows_are_independent_problems_bitwise(tmp_path_factory):
    """R = 3 rows in one call = three single-row calls, bit for bit (embedding observations, both compute modes)."""
    for compute in ("f32", "bf16"):
        g, mod = _module("cem_tacorl", compute, tmp_path_factory)
        c = g.case("n64_actor_twin")
        cem = _cem(g, mod, c)
        gen = torch.Generator().manual_seed(5)
        emb = g.emb("q1").float() + 0.05 * torch.randn(3, g.emb("q1").numel(), generator=gen)
        eps = torch.randn(3, 4, 64, 16, generator=gen)
        mean0 = 0.3 * torch.randn(3, 16, generator=gen)
        a3, t3 = cem.get_action(emb, initial_mean=mean0, noise={"eps": eps}, return_trace=True)
        assert a3.shape == (3, 16)
        for r in range(3):
            a1, t1 = cem.get_action(emb[r: r + 1], initial_mean=mean0[r: r + 1], noise={"eps": eps[r: r + 1]}, return_trace=True)
            assert torch.equal(a1[0], a3[r]), (compute, r)
            for k in t3:
                assert torch.equal(t1[k][0], t3[k][r]), (compute, r, k)
        assert not torch.equal(a3[0], a3[1])


def test_fresh_draws_give_a_valid_action(tmp_path_factory):
    g, mod = _module("cem_cql", "f32", tmp_path_factory)
    cem = _cem(g, mod, g.case("n256_actor"))
    obs = _to_dev(g.obs(True), mod.device)
    for twin in (False, True):
        cem.twin_min = twin
        a = cem.get_action(obs)
        assert a.shape == (1, 7) and torch.isfinite(a).all() and bool((a.abs() <= 1).all()) and abs(float(a[0, -1])) == 1.0
    a = cem.get_action(_to_dev(g.obs(False), mod.device))
    assert a.shape == (7,) and abs(float(a[-1])) == 1.0


def test_get_action_does_not_synchronise(tmp_path_factory):
    """Chosen check: get_action runs inside a torch.cuda.graph capture - a device-to-host copy or a synchronisation inside it
    would fail the capture - and the replayed graph reproduces the eager result."""
    g, mod = _module("cem_tacorl", "f32", tmp_path_factory)
    c = g.case("n64_actor_twin")
    cem = _cem(g, mod, c)
    dev = mod.device
    emb = g.emb("q1").float().to(dev).reshape(1, -1)
    noise = {"eps": c["eps"].to(dev).reshape(1, 4, 64, 16)}
    ref = cem.get_action(emb, noise=noise).clone()  # warm-up: the workspace exists
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = cem.get_action(emb, noise=noise)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_rollout_call_captures_with_images_and_device_draws(tmp_path_factory):
    """The call a rollout manager makes - image observation, the draws taken on the device, bf16 compute with its mirror
    refresh, twin minimum (both critics' encoders and goal encoders) - also runs inside a capture: no part of that path
    synchronises or copies to the host.  Only the capture and a valid replayed result are asserted (the draws are fresh)."""
    g, mod = _module("cem_cql", "bf16", tmp_path_factory)
    cem = _cem(g, mod, g.case("n256_zero_twin"))
    obs = _to_dev(g.obs(True), mod.device)
    cem.get_action(obs)  # warm-up: encoder buffers and workspace exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = cem.get_action(obs)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert out.shape == (1, 7) and torch.isfinite(out).all() and bool((out.abs() <= 1).all()) and abs(float(out[0, -1])) == 1.0


def test_bf16_refinement_after_training_steps_uses_the_current_weights():
    """Evaluation during training: after bf16 training steps (the optimiser kernels rewrite the fp32 masters through raw
    pointers, torch's version counters do not move) get_action must evaluate the CURRENT critics.  The trace's Q on the
    trace's own population agrees with the bf16-rounded Q head of the module's present state dict within 3e-2 - and is
    closer to it than to the Q head of the weights before the steps; module.q1(obs, a) sees the same weights."""
    from tacorl_amd import synth
    from tacorl_amd.lightning import instantiate
    from tacorl_amd.modules.cem import CEMOptimizer
    from tests.test_step_gpu import to_dev

    g = CemGolden("cem_cql")
    mod = instantiate(C.cql_cfg(device="cuda:0", compute_dtype="bf16", image_dtype="f32"))
    mod.load_state_dict(g.params())
    mod.current_epoch = 5  # Q phase: the critics move
    keys = [k for k in g.params() if k.startswith(("q1.critic.", "q2.critic."))]
    emb = g.emb("q1").float().reshape(1, -1)
    cem = CEMOptimizer(mod.q1, mod.q2, batch_size=64, action_dim=7, discrete_gripper=True, twin_min=True)
    eps = g.case("n64_zero_twin")["eps"]
    cem.get_action(emb, noise={"eps": eps})  # the mirrors are current for the initial weights
    before = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items() if k in keys}
    for step in range(8):
        mod.training_step(to_dev(synth.make_transition_batch(900 + step, 8, g.cams), mod.device), 0)
    torch.cuda.synchronize()
    after = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items() if k in keys}
    assert any(not torch.equal(before[k], after[k]) for k in keys)
    _, tr = cem.get_action(emb, noise={"eps": eps}, return_trace=True)
    pop, q = tr["pop"][0, 0].cpu(), tr["q"][0, 0].cpu()
    now = rel(q, q_fn_of(after, True, torch.float64, bf16_operands=True)((emb[0], emb[0]), pop.double()))
    old = rel(q, q_fn_of(before, True, torch.float64, bf16_operands=True)((emb[0], emb[0]), pop.double()))
    print(f"bf16 Q after 8 training steps: rel {now:.3g} to the current weights, {old:.3g} to the weights before")
    assert now < 3e-2 and now < old, (now, old)
    q1_surface = mod.q1(emb.to(mod.device), pop.to(mod.device)).reshape(-1).cpu()
    assert rel(q1_surface, q_head(after, "q1", torch.float64, bf16_operands=True)(emb[0], pop.double())) < 3e-2


def test_end_to_end_tacorl_plan_refinement(tmp_path_factory):
    """The rollout manager's use_cem sequence on TACORL built from a reference run directory: the actor's deterministic plan
    starts the refinement, the refined plan matches the fixture and drives the action decoder."""
    g, mod = _module("cem_tacorl", "f32", tmp_path_factory)
    c = g.case("n256_actor")
    obs = _to_dev(g.obs(True), mod.device)
    cem = _cem(g, mod, c)
    initial_mean, _ = mod.actor.get_actions(obs, deterministic=True, reparameterize=False)
    assert rel(initial_mean[0], c["mean0"]) < 1e-4
    plan = cem.get_action(obs=obs, initial_mean=initial_mean, noise={"eps": c["eps"]})
    assert plan.shape == (1, 16) and rel(plan[0], c["action"]) < 1e-4, rel(plan[0], c["action"])
    mod.action_decoder.clear_hidden_state()
    st = mod.perceptual_encoder.get_state_from_observation(obs["observation"], mod.action_decoder_modalities)
    a = mod.action_decoder.act(latent_plan=plan, perceptual_emb=st.unsqueeze(1))
    assert a.shape == (1, 1, 7) and torch.isfinite(a).all() and abs(float(a[0, 0, -1])) == 1.0


def test_end_to_end_cql_discrete_gripper(tmp_path_factory):
    g, mod = _module("cem_cql", "f32", tmp_path_factory)
    c = g.case("n256_actor")
    obs = _to_dev(g.obs(False), mod.device)
    cem = _cem(g, mod, c)
    assert mod.actor.discrete_gripper and cem.discrete_gripper
    initial_mean, _ = mod.actor.get_actions(obs, deterministic=True, reparameterize=False)
    assert rel(initial_mean[0], c["mean0"]) < 1e-4
    action = cem.get_action(obs=obs, initial_mean=initial_mean, noise={"eps": c["eps"]}).cpu().numpy()
    assert action.shape == (7,) and rel(action, c["action"]) < 1e-4 and float(action[-1]) == float(c["action"][-1])
