"""CQL_Offline on vector observations - drop-in for reference modules/cql/cql_offline_lightning_d4rl.py:23-492 (D4RL AntMaze).

Same constructor kwargs (`_recursive_: False`), `training_step / validation_step / configure_optimizers`, `state_dict()` keys
(`actor.policy.*`, `q1.Q.*`, `target_q1.Q.*`, `log_alpha`, `log_alpha_prime`) and logged scalar names as the reference; the
arithmetic is tacorl_amd.vec_engine.VecACEngine - the image module's step without an encoder stage.  The batch is the
reference's transition batch: `observations` / `next_observations` (B, state_dim + 2) with the goal already appended,
`actions` (B, action_dim), `rewards`, `terminals`.  Nothing imports gym or d4rl (modules/d4rl_env.py).
Select it with `module._target_=tacorl_amd.modules.cql.cql_offline_lightning_d4rl.CQL_Offline`.
"""
import torch.nn as nn

from ... import dist as _D
from ...lightning import LightningModuleBase
from ...vec_engine import VecACEngine
from ..common import register_views, to_plain
from ..d4rl_env import GOAL_DIM, env_dims
from .cql_offline_lightning import CQL_Offline as _ImageCQL


class CQL_Offline(_ImageCQL):
    def __init__(self, env={}, actor={}, critic={}, transform_manager={}, discount: float = 0.99, tau: float = 0.005,
                 actor_lr: float = 3e-4, critic_lr: float = 3e-4, deterministic_backup: bool = False,
                 reward_scale: float = 1.0, bc_epochs: int = 0, clip_grad: bool = True, clip_grad_val: int = 1,
                 conservative_weight: float = 1.0, lagrange_thresh: float = 5.0, n_action_samples: int = 10,
                 temp: float = 1.0, with_lagrange: bool = False, with_dr3: bool = False, dr3_coefficient: float = 0.03,
                 with_vib: bool = False, vib_coefficient: float = 0.01, d4rl_env: str = "antmaze-large-diverse-v0", *args,
                 state_dim=None, action_dim=None, device=None, compute_dtype="f32", world_size=1, device_noise_seed=None,
                 **kwargs):
        LightningModuleBase.__init__(self)
        if with_dr3:
            # (the reference's D4RL critics are plain `Critic`s without get_emb_obs_representation, which its DR3 term
            # calls: the reference itself fails with with_dr3=True on vector observations, so there is nothing to match)
            raise NotImplementedError("with_dr3=True: the reference's D4RL critics are plain Critics without "
                                      "get_emb_obs_representation, so the reference itself fails there; DR3 is built for "
                                      "the image modules only")
        if with_vib:
            raise NotImplementedError("the VIB regulariser is not built (with_vib=True; SURVEY 8a A9)")
        self._init_runtime(device, compute_dtype, "f32", world_size)
        self.automatic_optimization = False  # reference :95
        self.save_hyperparameters(ignore=["play_lmp"])  # reference :96
        self.d4rl_env, self.env, self.transform_manager = d4rl_env, None, transform_manager
        # the three facts the reference reads from gym.make(d4rl_env) (:57,133-137)
        self.state_dim, self.env_action_dim, self.act_bound = env_dims(d4rl_env, state_dim, action_dim)
        self.goal_dim = GOAL_DIM
        self.action_dim = self.env_action_dim
        self.bc_epochs, self.clip_grad = bc_epochs, clip_grad
        self.actor_lr, self.critic_lr = actor_lr, critic_lr
        self.with_lagrange = with_lagrange
        self.n_action_samples = n_action_samples
        self._hp = dict(discount=discount, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr,
                        deterministic_backup=deterministic_backup, reward_scale=reward_scale,
                        clip_grad_val=float(clip_grad_val) if clip_grad else 0.0,
                        conservative_weight=conservative_weight, lagrange_thresh=lagrange_thresh, temp=temp,
                        with_lagrange=with_lagrange, n=n_action_samples)
        self.actor_cfg, self.critic_cfg = to_plain(actor), to_plain(critic)
        self.obs_modalities, self.goal_modalities = [], []
        self.target_entropy = -float(self.env_action_dim)  # -prod(env.action_space.shape) (:76-78)
        self.build_networks()
        self.set_device_noise(device_noise_seed)
        if _D.collectives_on(world_size):
            self.sync_from_rank0()

    # ------------------------------------------------------------------ construction
    def build_networks(self):
        """reference :129-149."""
        a = self._arch()
        if a["discrete_gripper"]:
            raise NotImplementedError("the vector-observation actor has no discrete gripper")
        if a["hidden"] != (self.critic_cfg or {}).get("q_network", {}).get("hidden_dim", 256):
            raise NotImplementedError("actor and critic hidden sizes must match")
        # the batch delivers [state | goal] rows whole (the actor's input_dim is state_dim + goal_dim, :133-137)
        self._make_vec_engine(self.state_dim + self.goal_dim, 0, self.action_dim, a)
        from ...init import init_views_

        e = self.engine
        for blk in (e.actor, e.q1, e.q2):
            init_views_(blk.views)
        self.sync_targets()
        self._register()
        self._attach_rollout()

    def _attach_rollout(self, ad=None):
        """Rollout surface (evaluation/rollout_manager_d4rl.py:183-222): actor.get_actions on [obs | goal] rows, callable
        critics (modules/cem.py takes them), the action decoder's one-step act where the module has a decoder."""
        from ..inference import attach_vec_rollout_surface

        e = self.engine
        attach_vec_rollout_surface(self, self.action_dim, actor_net=e.actor,
                                   critics={"q1": e.q1, "q2": e.q2, "target_q1": e.tq1, "target_q2": e.tq2}, ad=ad)

    def _make_vec_engine(self, state_dim, goal_dim, action_dim, a):
        hp = self._hp
        self.engine = VecACEngine(
            state_dim, goal_dim, action_dim, None, self.dev, n=hp["n"], discount=hp["discount"], tau=hp["tau"],
            actor_lr=hp["actor_lr"], critic_lr=hp["critic_lr"], deterministic_backup=hp["deterministic_backup"],
            reward_scale=hp["reward_scale"], clip_grad_val=hp["clip_grad_val"], conservative_weight=hp["conservative_weight"],
            lagrange_thresh=hp["lagrange_thresh"], temp=hp["temp"], with_lagrange=hp["with_lagrange"],
            target_entropy=self.target_entropy, policy_layers=a["policy_layers"], q_layers=a["q_layers"], hidden=a["hidden"],
            compute=self.compute, world_size=self.world_size)

    def _register(self):
        e = self.engine
        self._pv = {}  # block name -> {view name: Parameter}: what the BlockAdams are built from
        for name, blk in (("actor", e.actor), ("q1", e.q1), ("q2", e.q2), ("target_q1", e.tq1), ("target_q2", e.tq2)):
            self._pv[name] = register_views(self, name + ".", blk.views)
        self.log_alpha = nn.Parameter(e.log_alpha.param)
        if self.with_lagrange:
            self.log_alpha_prime = nn.Parameter(e.log_alpha_prime.param)

    # ---------------------------------------------------------------------- stepping
    def overwrite_batch(self, batch):
        """reference :98-127."""
        return (batch["observations"].float(), batch["actions"].float(), batch["next_observations"].float(),
                batch["rewards"].float(), batch["terminals"].int())

    def compute_update(self, batch, optimize: bool = True, log_type: str = "train", noise=None):
        import torch

        obs, action, nxt, reward, done = batch
        self._sync_lrs()
        e, dev = self.engine, self.dev
        B = action.shape[0]
        e.ensure_batch(B, 2)
        # a transition is a window of two observations whose goal columns are part of the rows (:133-137: the actor's input
        # is state_dim + goal_dim wide and the batch delivers it whole)
        e.load_observations(torch.stack([obs.to(dev), nxt.to(dev)], 1))
        e.load_transition(action.to(dev), reward.to(dev), done.to(dev))
        e.set_noise(noise)
        bc = self.current_epoch < self.bc_epochs
        self._run_segments(("cql_d4rl", B, bc, optimize),
                           [lambda: e.phase_a(optimize=optimize), lambda: e.phase_b(bc, optimize), lambda: e.phase_c(optimize)],
                           [e.allreduce_alpha, e.allreduce_grads])
        self._publish_logs(log_type)
