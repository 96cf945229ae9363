"""The actor-critic update on vector observations (reference modules/cql/cql_offline_lightning_d4rl.py:388-460,
modules/tacorl/tacorl_d4rl.py:68-89 - D4RL AntMaze: state 29, goal 2): ACEngine's step without an encoder stage.

The state rows of the policy and Q chains come straight from the batch - `observations (B,T,S)` and `goal (B,G)`, the rows
[observations[:,0] | goal] and [observations[:,-1] | goal] - so there are no image slots, no encoders, no goal-encoder block and
no encoder backward: the five networks are their head MLPs alone, the MLP backward stops at the heads, and the only input
gradient the step computes is the actor's through the critics' action columns.  One launch (tacorl_vec_rows) writes the policy
rows in the first phase, one writes every Q input row in the second; the actor, q1 and q2 read the same rows (as do the
actor on next and the two targets), so each exists once.  Phases, losses, optimiser steps and collectives are ACEngine's.
"""
import torch

from . import blocks, ops
from ._lib import F32, call, ptr
from .engine import ACEngine, NetBlock, _al4


class HeadBlock(NetBlock):
    """A network that is its head MLP alone, in one flat buffer (no encoders, no goal encoder in front of it)."""

    genc_dims = genc_acts = ()

    def __init__(self, head_dims, head_acts, head_names, device, head_parts=None):
        self.cams = self.goal_cams = self.all_cams = []
        self.enc_off = {}
        self.genc_off = self.head_off = 0  # (the bf16 mirror of "the MLP part" is the whole block)
        self.head_dims, self.head_acts = list(head_dims), list(head_acts)
        self.size = blocks.mlp_size(self.head_dims)
        self._head_names, self._head_parts = head_names, head_parts
        self._alloc_block(device)

    def _views_of(self, flat):
        return self._head_views(flat)


class VecACEngine(ACEngine):
    name_prefix = ("", "")  # policy.* / Q.* as the reference's Actor and Critic name them (no visual wrapper around them)

    def __init__(self, state_dim, goal_dim, action_dim, B, device, *, n=4, discount=0.99, tau=0.005, actor_lr=3e-4,
                 critic_lr=3e-4, deterministic_backup=False, reward_scale=1.0, clip_grad_val=1.0, conservative_weight=1.0,
                 lagrange_thresh=5.0, temp=1.0, with_lagrange=False, target_entropy=-8.0, policy_layers=3, q_layers=3,
                 hidden=256, compute=F32, world_size=1):
        if state_dim < 1 or goal_dim < 0 or action_dim < 1:
            raise ValueError(f"state_dim {state_dim}, goal_dim {goal_dim}, action_dim {action_dim}")
        self.cams, self.goal_cams, self.enc_cams, self.hw = [], [], [], {}
        self.img_dtype = torch.float32
        self.Sd, self.G = state_dim, goal_dim
        self.Eo = self.E = state_dim + goal_dim
        self.lds = _al4(self.E)  # the rows' leading dimension (16-byte rows for the chains' vector loads); pad columns are zero
        self.T = 2
        self._init_step(action_dim, B, device, n, dict(
            discount=discount, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr, deterministic_backup=deterministic_backup,
            reward_scale=reward_scale, clip=clip_grad_val, cons_w=conservative_weight, gap=lagrange_thresh, temp=temp,
            target_entropy=target_entropy), with_lagrange, False, policy_layers, q_layers, hidden, compute, world_size)

    def _net_block(self, head_dims, head_acts, head_names, head_parts):
        return HeadBlock(head_dims, head_acts, head_names, self.dev, head_parts=head_parts)

    # ------------------------------------------------------------------ buffers
    def ensure_batch(self, B, T=None):
        """(Re)allocate every batch-sized buffer for B windows of T observations (a transition is a window of 2)."""
        T = self.T if T is None else T
        if self.B != B or self.T != T:
            self.B, self.T = B, T
            self._alloc()

    def _alloc_encoder_stage(self):
        """No stage: the batch's observations and goals, and the rows the one-launch assembly writes from them."""
        B, dev = self.B, self.dev
        f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        self.obs, self.goal = f(B, self.T, self.Sd), f(B, max(self.G, 1))
        s, nx = f(B, self.lds), f(B, self.lds)
        self.S = {"a": s, "q1": s, "q2": s, "a_nx": nx, "tq1": nx, "tq2": nx}
        xq, xqpi, xt = f((3 * self.n + 1) * B, self.ldq), f(B, self.ldq), f(B, self.ldq)
        self.XQ, self.XQpi, self.XT = {"q1": xq, "q2": xq}, {"q1": xqpi, "q2": xqpi}, {"tq1": xt, "tq2": xt}
        # the backward stops at the heads: no input gradient of the policy rows or of the R Q rows is formed
        self.dS, self.dXQ = {"a": None}, {"q1": None, "q2": None}

    def load_observations(self, observations, goal=None):
        """observations (B,T,S): the window whose first and last entries are obs and next; goal (B,G), or None with G = 0."""
        self.obs.copy_(observations.reshape(self.obs.shape))
        if self.G:
            self.goal.copy_(goal.reshape(self.goal.shape))

    def load_images(self, *a, **k):
        raise NotImplementedError("the vector-observation step has no image slots")

    # ----------------------------------------------------------------- forward
    def _encode_all(self):
        pass

    def packs_stale(self):
        return False

    def packs_written(self):
        pass

    def _gather_ok(self, tag):
        return False  # (the rows are written once by tacorl_vec_rows; nothing is left to gather)

    def _vec_rows(self, out):
        call("tacorl_vec_rows", ptr(self.obs), ptr(self.goal) if self.G else None, ptr(self.acts_main), ptr(self.act_pi),
             ptr(self.act_next), ops.ptr_array(out), None, self.B, self.T, self.Sd, self.G, self.A, self.n, self.lds, self.ldq,
             ops.stream())

    def _assemble_states(self):
        self._vec_rows([self.S["a"], self.S["a_nx"], None, None, None])

    def _assemble_q_rows(self):
        self._vec_rows([None, None, self.XQ["q1"], self.XQpi["q1"], self.XT["tq1"]])

    # ---------------------------------------------------------------- backward
    def _mlp_bwd_sites(self):
        return [site for site in super()._mlp_bwd_sites() if site[0] != "genc"]

    def _ebw_sequences(self):
        return []

    def _state_grads_from_q(self):
        pass

    def _encoders_backward(self):
        pass
