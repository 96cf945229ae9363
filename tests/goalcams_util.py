"""Shared by tests/test_goalcams_cpu.py, tests/test_goalcams_gpu.py and tests/goalcams_rccl_script.py: CQL_Offline with goal
cameras that differ from the observation cameras (fixture tests/golden/cql_goalcams.npz, oracle/gen_goalcams_golden.py)."""
import torch

from tacorl_amd import synth

NAME = "cql_goalcams"
ACTOR = {"policy": {"num_layers": 3, "hidden_dim": 256}}
CRITIC = {"q_network": {"num_layers": 3, "hidden_dim": 256, "last_layer_activation": "Identity"}}
# config/module/cql_offline_goal_cond.yaml:11-27 (as tests/test_step_gpu.py CQL_YAML)
CQL_YAML = dict(discount=0.99, actor_lr=1e-4, critic_lr=3e-4, conservative_weight=1.0, n_action_samples=4,
                with_lagrange=True, reward_scale=10.0, deterministic_backup=False, bc_epochs=5)
GEOM = {"rgb_static": (84, 84), "rgb_gripper": (64, 64)}


def spec_of(obs, goal):
    """ACSpec equal to what the module below (and the reference module of the fixture) is built with."""
    from oracle import tacorl_oracle as O

    return O.ACSpec(cams=list(obs), goal_cams=list(goal), action_dim=7, discrete_gripper=True, target_entropy=-7.0, n=4,
                    discount=0.99, actor_lr=1e-4, critic_lr=3e-4, deterministic_backup=False, reward_scale=10.0, bc_epochs=5,
                    with_lagrange=True)


def build(obs, goal, compute="f32", **kw):
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    return CQL_Offline(actor=dict(ACTOR, discrete_gripper=True), critic=CRITIC, real_world=True, obs_modalities=list(obs),
                       goal_modalities=list(goal), action_dim=7, device="cuda:0", compute_dtype=compute, image_dtype=compute,
                       **dict(CQL_YAML, **kw))


def synth_params(mod, seed):
    """synth values for every tensor of the module's own state dict (reference names, logical shapes)."""
    return {k: synth.param_values(k, tuple(v.shape), seed) for k, v in mod.state_dict().items() if v.dtype == torch.float32}


def synth_noise(seed, B, n=4, A=7):
    """The draws of one CQL_Offline step with the discrete gripper (names: golden_util.Golden.noise)."""
    gen = torch.Generator().manual_seed(seed)
    nrm = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    uni = lambda *s: torch.rand(*s, generator=gen).clamp(1e-6, 1 - 1e-6)  # noqa: E731
    Ac = A - 1
    return dict(eps_pi=nrm(B, Ac), g_pi=uni(B, 2), eps_next=nrm(B, Ac), g_next=uni(B, 2), u_rand=uni(n * B, A),
                eps_cur=nrm(n, B, Ac), g_cur=uni(n, B, 2), eps_nxt=nrm(n, B, Ac), g_nxt=uni(n, B, 2))


# ---- rollout surfaces: one observation, parameters as the CEM fixtures scale them (tests/golden/cem_cql.npz: the Q heads'
# output layer times 8, so that the reference's own Q values keep the elite boundary and the best candidate apart)
SURF_SEED, CEM_EPS_SEED, CEM_OUT_SCALE, CEM_N, CEM_ITERS, CEM_ELITE = 71, 7100002, 8.0, 64, 4, 6
CEM_GAP, CEM_ORDER_GAP = 1e-3, 1e-4  # the CEM fixtures' `gap` / `order_gap`


def surface_params(names_shapes, seed=SURF_SEED):
    P = {k: synth.param_values(k, s, seed) for k, s in names_shapes.items()}
    for k in P:
        if k.startswith(("q1.", "q2.")) and ".critic.Q.out." in k:
            P[k] = P[k] * CEM_OUT_SCALE
    return P


def surface_restatement(P, obs, spec):
    """The restatement's embeddings (actor, q1, q2), deterministic action and twin-min CEM trace for the observation."""
    from oracle import tacorl_oracle as O
    from tacorl_amd.modules.cem import cem_restatement
    from tests.cem_util import q_fn_of

    with torch.no_grad():
        emb = {n: O._emb(P, n + ".", obs["observation"], obs["goal"], spec) for n in ("actor", "q1", "q2")}
        mu, _, logits = O.policy(P, "actor.actor.policy.", emb["actor"], discrete_gripper=True)
        a_det = torch.cat([torch.tanh(mu), logits.argmax(-1, keepdim=True).float() * 2 - 1], dim=-1)
        eps = torch.randn(CEM_ITERS, CEM_N, 7, generator=torch.Generator().manual_seed(CEM_EPS_SEED))
        act, tr = cem_restatement(q_fn_of(P, True), (emb["q1"][0], emb["q2"][0]), a_det[0].double(), eps.double(),
                                  n_elite=CEM_ELITE, discrete_gripper=True)
    return emb, a_det, eps, act, tr
