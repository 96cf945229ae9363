"""Rollout-time surface of the module classes (reference evaluation/rollout_manager.py:310-431):
`module.actor.get_actions(obs, deterministic, reparameterize)` (actor.py:65-111 through
visual_actor_wrapper.py:41-76), `module.perceptual_encoder.get_state_from_observation(observation, modalities)`
(representation_network.py:36-71), `module.action_decoder.act / clear_hidden_state`
(action_decoder_logistic.py:73-97), and the critics `module.q1(obs, action)` / `q2` / `target_q1` / `target_q2` with
`get_emb_representation` / `get_emb_obs_representation` (visual_critic_wrapper.py:35-75), which CEM refinement
(modules/cem.py) is built on.  Small-batch latency path on the library's per-layer kernels (any number of
images, any camera geometry); nothing here is captured in a graph or keeps gradients.
"""
import torch

from .. import ops
from .._lib import BF16, F32, call, ptr


class EncoderRunner:
    """LMPVisionEncoder forward of N images through one network block (reference encoder.py:369-419)."""

    def __init__(self, owner):
        self.owner = owner
        self._buf = {}

    def _buffers(self, n, hw):
        key = (n, hw)
        if key not in self._buf:
            o = self.owner
            ops.note_alloc()
            self._buf[key] = (torch.zeros(n, *hw, 3, device=o.dev, dtype=o.img_dtype), torch.zeros(n, 32, device=o.dev),
                              torch.zeros(ops.encoder_act_layout(n, *hw)[1], device=o.dev))
        return self._buf[key]

    def encode(self, enc_ptr, images):
        """images (N,3,H,W) or (3,H,W) fp32 in [-1,1] (the transformed observation) -> (N,32) embeddings."""
        o = self.owner
        x = images.to(o.dev, torch.float32)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        x = x.contiguous()
        n, _, H, W = x.shape
        img, out, act = self._buffers(n, (H, W))
        xd = BF16 if o.img_dtype == torch.bfloat16 else F32
        call("tacorl_pack_images", ptr(x), 3 * H * W, 1, ptr(img), xd, n, 3, H, W, ops.stream())
        call("tacorl_encoder_fwd", 1, ops.ptr_array([img]), ops.ptr_array([enc_ptr]), ops.ptr_array([out]),
             ops.ptr_array([act]), ops.int_array([n]), H, W, xd, o.compute, ops.stream())
        # a copy, not the cached buffer: two cameras of one geometry (or obs and goal) share (n, hw) and hence `out`
        return out.clone()


def state_from_observation(owner, runner, net, observation, modalities, cat_output=True):
    """LateFusion.get_state_from_observation: per-camera embeddings concatenated in `modalities` order, or - with
    cat_output=False (representation_network.py:60-71) - the {camera: embedding} dict."""
    embs = [runner.encode(net.enc(c), observation[c]) for c in modalities]
    if not cat_output:
        return dict(zip(modalities, embs))
    return embs[0] if len(embs) == 1 else torch.cat(embs, dim=-1)


def _rows(x, dev):
    """(rows (n, E) fp32 on the device, unbatched?) of an embedding given as (n, E) or (E,)."""
    x = x.to(dev, torch.float32)
    return (x.unsqueeze(0), True) if x.dim() == 1 else (x, False)


def _mlp_rows(owner, x, ptr_, dims, acts):
    """One MLP chain of the library on rows x (n, dims[0]); returns the (n, dims[-1]) output (a fresh tensor)."""
    n, ld = x.shape[0], (dims[0] + 3) // 4 * 4
    if x.shape[1] != dims[0]:
        raise ValueError(f"the network takes {dims[0]} input columns, got {x.shape[1]}")
    xin = torch.zeros(n, ld, device=owner.dev)  # rows of whole 16-byte words, pad columns zero (the chains' vector loads)
    xin[:, :dims[0]] = x
    lay = ops.mlp_act_layout(n, dims, acts)
    act = torch.zeros(lay[2], device=owner.dev)
    ops.mlp_fwd([xin], ld, [ptr_], [act], [n], dims, acts, owner.compute)
    yo = lay[1][-1]
    return act[yo: yo + n * dims[-1]].view(n, dims[-1]).clone()


LOG_SIG_MIN, LOG_SIG_MAX, MEAN_MIN, MEAN_MAX = -5.0, 2.0, -9.0, 9.0  # reference actor.py:12-15


class TanhNormalDist:
    """What `get_dist` returns: the reference's TanhNormal (utils/distributions.py:61-153) by its attribute names -
    normal_mean (the clamped mean), normal_std (exp of the clamped log_std), mean = tanh(normal_mean), stddev - with the draws
    through the library's sampling kernel.  Holds the policy head as computed; keeps no gradient."""

    def __init__(self, head, A, unbatched=False):
        self._head, self._A, self._unbatched = head, A, unbatched
        sq = (lambda t: t[0]) if unbatched else (lambda t: t)
        self.normal_mean = sq(head[:, :A].clamp(MEAN_MIN, MEAN_MAX))
        self.normal_std = sq(head[:, A:2 * A].clamp(LOG_SIG_MIN, LOG_SIG_MAX).exp())

    @property
    def mean(self):
        return torch.tanh(self.normal_mean)

    @property
    def stddev(self):
        return self.normal_std

    def _draw(self, noise, reparameterize):
        head, A = self._head, self._A
        n, dev = head.shape[0], head.device
        eps = torch.randn(n, A, device=dev) if noise is None else noise.to(dev, torch.float32).reshape(n, A).contiguous()
        act, logp = torch.zeros(n, A, device=dev), torch.zeros(n, device=dev)
        ops.tanh_normal_sample(head, head.shape[1], eps, None, bool(reparameterize), act, 0, A, logp, None, 1, n, A)
        return (act[0] if self._unbatched else act), logp

    def sample(self, noise=None):
        """tanh(normal_mean + normal_std * eps); noise: the N(0,1) draws (n, A)."""
        return self._draw(noise, False)[0]

    def rsample(self, noise=None):
        return self._draw(noise, True)[0]

    def sample_and_logprob(self, noise=None):
        a, lp = self._draw(noise, False)
        return a, (lp if self._unbatched else lp.view(-1, 1))


class PlanProposalSurface:
    """Bound onto `module.plan_proposal`: Actor.get_dist (actor.py:50-63) over one network block's head MLP."""

    def __init__(self, owner, net, action_dim):
        self.owner, self.net, self.A = owner, net, int(action_dim)

    def get_dist(self, state_emb, goal_emb=None):
        """state_emb (n, S) or (S,), goal_emb (n, G) / (G,) or None (state_emb then holds both) -> TanhNormalDist."""
        s, unb = _rows(state_emb, self.owner.dev)
        if goal_emb is not None:
            s = torch.cat([s, _rows(goal_emb, self.owner.dev)[0]], dim=-1)
        head = _mlp_rows(self.owner, s, self.net.head(), self.net.head_dims, self.net.head_acts)
        return TanhNormalDist(head, self.A, unb)


class VecActorSurface:
    """Bound onto `module.actor` of the vector-observation modules: Actor.get_actions (actor.py:65-111) on [state | goal]
    rows (n, E) or one row (E,) (evaluation/rollout_manager_d4rl.py:207-222)."""

    def __init__(self, owner, net, action_dim):
        self.pp = PlanProposalSurface(owner, net, action_dim)
        self.A = int(action_dim)

    def emb_representation(self, obs):
        return obs.to(self.pp.owner.dev, torch.float32)

    def get_actions(self, observation, deterministic=False, reparameterize=False, noise=None):
        """Returns (actions, log_pi): log_pi is zeros_like(actions) when deterministic, (n, 1) otherwise.
        noise: {'eps': (n, A) N(0,1)} injects the draws."""
        d = self.pp.get_dist(observation)
        if deterministic:
            # tanh(mean): the sampling kernel with eps = 0
            a = d.sample(noise=torch.zeros(d._head.shape[0], self.A, device=d._head.device))
            return a, torch.zeros_like(a)
        a, lp = d._draw(noise["eps"] if noise else None, reparameterize)
        return a, (lp if d._unbatched else lp.view(-1, 1))


def attach_vec_rollout_surface(module, action_dim, actor_net=None, critics=None, plan_proposal_net=None, ad=None):
    """The vector-observation modules' rollout methods under the reference's names: `actor.get_actions`, callable critics
    (which CEMOptimizer accepts), `plan_proposal.get_dist`, `action_decoder.act / clear_hidden_state`."""
    if actor_net is not None:
        surf = VecActorSurface(module, actor_net, action_dim)
        module.__dict__["_actor_surface"] = surf
        module.actor.get_actions = surf.get_actions
        module.actor.get_dist = surf.pp.get_dist
        module.actor.get_emb_representation = surf.emb_representation
        module.actor.action_dim = int(action_dim)
        module.actor.discrete_gripper = False
    for name, net in (critics or {}).items():
        cs = CriticSurface(module, net, [], [], action_dim)
        box = getattr(module, name)
        box.forward = cs.forward
        box.get_emb_representation = cs.emb_representation
        box.get_emb_obs_representation = cs.emb_obs_representation
        box.__dict__["critic_surface"] = cs
    if plan_proposal_net is not None:
        pp = PlanProposalSurface(module, plan_proposal_net, action_dim)
        module.__dict__["_plan_proposal_surface"] = pp
        module.plan_proposal.get_dist = pp.get_dist
    if ad is not None:
        module.action_decoder.clear_hidden_state = ad.clear_hidden_state
        module.action_decoder.act = lambda latent_plan, perceptual_emb, latent_goal=None, noise=None: ad.act(
            latent_plan, perceptual_emb, latent_goal, noise=noise, compute=module.compute)


def attach_goal_encoder(module, net):
    """`module.goal_encoder(x)`: the goal-encoder MLP of one network block on embeddings (n, 32 per camera) or one row."""
    def forward(x):
        rows, unb = _rows(x, module.dev)
        y = _mlp_rows(module, rows, net.genc(), net.genc_dims, net.genc_acts)
        return y[0] if unb else y

    module.goal_encoder.forward = forward


class ActorSurface:
    """Bound onto `module.actor`: get_actions of VisualActorWrapper + Actor + MLPPolicy for one network block."""

    def __init__(self, owner, net, cams, goal_cams, action_dim, discrete_gripper):
        self.owner, self.net, self.cams, self.goal_cams = owner, net, list(cams), list(goal_cams)
        self.A, self.dg = action_dim, bool(discrete_gripper)
        self.Ac = action_dim - 1 if self.dg else action_dim
        self.HD = 2 * self.Ac + (2 if self.dg else 0)
        self.runner = EncoderRunner(owner)
        self._buf = {}

    def emb_representation(self, obs):
        """[enc(obs) | goal_encoder(enc(goal))] (visual_actor_wrapper.py:41-62); a tensor passes through."""
        if not isinstance(obs, dict):
            return obs.to(self.owner.dev, torch.float32)
        o, net = self.owner, self.net
        if "goal" not in obs:
            return state_from_observation(o, self.runner, net, obs.get("observation", obs), self.cams)
        e_obs = state_from_observation(o, self.runner, net, obs["observation"], self.cams)
        e_goal = state_from_observation(o, self.runner, net, obs["goal"], self.goal_cams)
        n = e_obs.shape[0]
        gact = torch.zeros(ops.mlp_act_layout(n, net.genc_dims, net.genc_acts)[2], device=o.dev)
        ops.mlp_fwd([e_goal], e_goal.shape[1], [net.genc()], [gact], [n], net.genc_dims, net.genc_acts, o.compute)
        yo = ops.mlp_act_layout(n, net.genc_dims, net.genc_acts)[1][-1]
        return torch.cat([e_obs, gact[yo: yo + n * net.G].view(n, net.G)], dim=-1)

    def get_actions(self, observation, deterministic=False, reparameterize=False, noise=None):
        """actor.py:65-111.  Returns (actions (N,A), log_pi): log_pi is zeros_like(actions) when deterministic, (N,1)
        otherwise.  noise: {'eps': (N,Ac) N(0,1)[, 'gumbel_u': (N,2) U(0,1)]} injects the draws."""
        o, net = self.owner, self.net
        s = self.emb_representation(observation).contiguous()
        n = s.shape[0]
        pact = torch.zeros(ops.mlp_act_layout(n, net.head_dims, net.head_acts)[2], device=o.dev)
        ops.mlp_fwd([s], s.shape[1], [net.head()], [pact], [n], net.head_dims, net.head_acts, o.compute)
        yo = ops.mlp_act_layout(n, net.head_dims, net.head_acts)[1][-1]
        head = pact[yo: yo + n * self.HD]
        f = lambda *sh: torch.zeros(*sh, device=o.dev)  # noqa: E731
        act, logp = f(n, self.A), f(n)
        if deterministic:
            # tanh(mean) and the argmax gripper class = the sampling kernel with eps = 0 and equal Gumbel noise
            eps, gu = f(n, self.Ac), torch.full((n, 2), 0.5, device=o.dev) if self.dg else None
        else:
            eps = noise["eps"].to(o.dev).reshape(n, self.Ac).contiguous() if noise else torch.randn(n, self.Ac, device=o.dev)
            gu = None
            if self.dg:
                gu = noise["gumbel_u"].to(o.dev).reshape(n, 2).contiguous() if noise else torch.rand(n, 2, device=o.dev)
        grip = torch.zeros(n, dtype=torch.int32, device=o.dev) if self.dg else None
        ops.tanh_normal_sample(head, self.HD, eps, gu, bool(reparameterize and not deterministic), act, 0, self.A, logp, grip,
                               1, n, self.Ac)
        if deterministic:
            return act, torch.zeros_like(act)
        return act, logp.view(n, 1)


class CriticSurface:
    """Bound onto `module.q1` (q2, target_q1, target_q2): VisualCriticWrapper + Critic + MLPQNetwork of one network block.
    Calling the container returns Q(obs, action) as (n, 1)."""

    def __init__(self, owner, net, cams, goal_cams, action_dim, runner=None):
        self.owner, self.net, self.cams, self.goal_cams = owner, net, list(cams), list(goal_cams)
        self.A = int(action_dim)
        self.E = net.head_dims[0] - self.A
        self.hidden, self.q_layers = net.head_dims[1], len(net.head_dims) - 2
        self.runner = runner or EncoderRunner(owner)

    def emb_obs_representation(self, obs):
        """The observation's embedding without the goal (visual_critic_wrapper.py:35-48); a tensor passes through."""
        if not isinstance(obs, dict):
            return obs.to(self.owner.dev, torch.float32)
        od = obs["observation"] if self.goal_cams and "goal" in obs else obs
        return state_from_observation(self.owner, self.runner, self.net, od, self.cams)

    def emb_representation(self, obs):
        """[enc(obs) | goal_encoder(enc(goal))] with this critic's own encoders (visual_critic_wrapper.py:50-71)."""
        if not isinstance(obs, dict):
            return obs.to(self.owner.dev, torch.float32)
        o, net = self.owner, self.net
        if not (self.goal_cams and "goal" in obs):
            return state_from_observation(o, self.runner, net, obs, self.cams)
        e_obs = state_from_observation(o, self.runner, net, obs["observation"], self.cams)
        e_goal = state_from_observation(o, self.runner, net, obs["goal"], self.goal_cams)
        n = e_obs.shape[0]
        gact = torch.zeros(ops.mlp_act_layout(n, net.genc_dims, net.genc_acts)[2], device=o.dev)
        ops.mlp_fwd([e_goal], e_goal.shape[1], [net.genc()], [gact], [n], net.genc_dims, net.genc_acts, o.compute)
        yo = ops.mlp_act_layout(n, net.genc_dims, net.genc_acts)[1][-1]
        return torch.cat([e_obs, gact[yo: yo + n * net.G].view(n, net.G)], dim=-1)

    def forward(self, obs, action):
        """critic.py:92-97 on [embedding | action].  Images (n,3,H,W) or (3,H,W), an embedding (n,E) or (E,), actions (n,A)
        or (A,); one observation row is shared by all action rows (the reference's expand_obs).  Returns (n, 1)."""
        o, net = self.owner, self.net
        s = self.emb_representation(obs)
        s = s.unsqueeze(0) if s.dim() == 1 else s
        a = action.to(o.dev, torch.float32)
        a = a.unsqueeze(0) if a.dim() == 1 else a
        if s.shape[1] != self.E or a.shape[1] != self.A:
            raise ValueError(f"critic takes an embedding of {self.E} and an action of {self.A} columns, got {s.shape[1]} and "
                             f"{a.shape[1]}")
        n = a.shape[0]
        if s.shape[0] not in (1, n):
            raise ValueError(f"{s.shape[0]} observation rows for {n} action rows")
        ldx = (self.E + self.A + 3) // 4 * 4
        x = torch.zeros(n, ldx, device=o.dev)
        x[:, :self.E] = s
        x[:, self.E: self.E + self.A] = a
        qact = torch.zeros(ops.mlp_act_layout(n, net.head_dims, net.head_acts)[2], device=o.dev)
        ops.mlp_fwd([x], ldx, [net.head()], [qact], [n], net.head_dims, net.head_acts, o.compute)
        yo = ops.mlp_act_layout(n, net.head_dims, net.head_acts)[1][-1]
        return qact[yo: yo + n].view(n, 1).clone()

    __call__ = forward


def attach_rollout_surface(module, actor_net, cams, goal_cams, action_dim, discrete_gripper, lmp_net=None, lmp_cams=None,
                           ad=None, critics=None):
    """Give the module's reference-named containers their rollout methods.  critics: {container name: network block}."""
    if critics:
        runner = EncoderRunner(module)
        for name, net in critics.items():
            cs = CriticSurface(module, net, cams, goal_cams, action_dim, runner)
            box = getattr(module, name)
            box.forward = cs.forward  # nn.Module.__call__ finds the instance attribute: module.q1(obs, action)
            box.get_emb_representation = cs.emb_representation
            box.get_emb_obs_representation = cs.emb_obs_representation
            box.__dict__["critic_surface"] = cs
    surf = ActorSurface(module, actor_net, cams, goal_cams, action_dim, discrete_gripper)
    module.__dict__["_actor_surface"] = surf
    module.actor.get_actions = surf.get_actions
    module.actor.get_emb_representation = surf.emb_representation
    module.actor.action_dim = action_dim
    module.actor.discrete_gripper = bool(discrete_gripper)
    if lmp_net is not None:
        runner = EncoderRunner(module)
        module.__dict__["_pe_runner"] = runner
        module.perceptual_encoder.get_state_from_observation = (
            lambda observation, modalities=None, cat_output=True: state_from_observation(
                module, runner, lmp_net, observation, list(modalities or lmp_cams), cat_output))
    if ad is not None:
        module.action_decoder.clear_hidden_state = ad.clear_hidden_state
        module.action_decoder.act = lambda latent_plan, perceptual_emb, latent_goal=None, noise=None: ad.act(
            latent_plan, perceptual_emb, latent_goal, noise=noise, compute=module.compute)


# ---------------------------------------------------------------------------------- relay imitation learning
class RILNetView:
    """One network of the relay-imitation block (RILBlock: one encoder per camera, one goal encoder, two policies) in the
    form the surfaces above read a network block: `enc(cam)`, `genc() / genc_dims / genc_acts / G` and - for key "high" or
    "low" - that policy's `head() / head_dims / head_acts`."""

    def __init__(self, engine, key=None):
        blk = engine.blk
        self.enc, self.genc = blk.enc, blk.genc
        self.genc_dims, self.genc_acts, self.G = list(engine.genc_dims), list(engine.genc_acts), engine.GO
        self.key = key
        if key is not None:
            self.head = lambda: blk.pol(key)
            self.head_dims, self.head_acts = list(engine.pol_dims[key]), list(engine.pol_acts[key])
            self.Ac, self.dg = engine.Ac[key], bool(engine.dg) if key == "low" else False
            self.A = self.Ac + int(self.dg)


class RowsMLP:
    """One MLP chain of the library for 1 .. max_rows (<= 64) rows on buffers allocated once - the rollout's inner loop.
    route "rows": ONE tacorl_rows_mlp_fwd call (csrc/rollout_ops.hip), fp32 from the masters; route "composed": the training
    chain ops.mlp_fwd in fp32 and, for a policy head, ops.tanh_normal_sample with eps = 0 and equal Gumbel noise.
    policy: None (the last layer is an ordinary one: mode "plain") or (Ac, discrete_gripper): the output is the (n, Ac + dg)
    deterministic action."""

    def __init__(self, owner, base, dims, acts, max_rows, policy=None):
        self.dev, self.base, self.dims, self.acts, self.R = owner.dev, base, list(dims), list(acts), int(max_rows)
        self.policy = None if policy is None else (int(policy[0]), bool(policy[1]))
        self.n_out = self.dims[-1] if policy is None else self.policy[0] + int(self.policy[1])
        self.wo, self.bo, _ = ops.mlp_param_layout(self.dims)
        self._c_dims, self._c_acts = ops.int_array(self.dims), ops.int_array(self.acts)
        self._at, self._w, self._b = None, None, None
        ops.note_alloc()
        f = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
        self.ws = f(max(self.R * sum(self.dims[1:-1]), 1))
        self.act = f(ops.mlp_act_layout(self.R, self.dims, self.acts)[2])
        if self.policy is not None:
            Ac, dg = self.policy
            self.eps, self.logp = f(self.R, Ac), f(self.R)
            self.gu = torch.full((self.R, 2), 0.5, device=self.dev) if dg else None
            self.grip = torch.zeros(self.R, dtype=torch.int32, device=self.dev) if dg else None
        self._yoff = {}

    def supported(self, n):
        Ac, dg = self.policy or (0, False)
        return bool(ops.L.lib().tacorl_rows_mlp_supported(int(n), len(self.acts), self._c_dims, int(self.policy is not None),
                                                          Ac, int(dg)))

    def _params(self):
        base = self.base()
        if base != self._at:
            n = len(self.acts)
            self._w = (ops.C.c_void_p * n)(*[base + 4 * o for o in self.wo])
            self._b = (ops.C.c_void_p * n)(*[base + 4 * o for o in self.bo])
            self._at = base
        return base

    def hidden(self, n, l):
        """Layer l's (n, dims[l+1]) output of the last "rows" call of n rows."""
        o = n * sum(self.dims[1: l + 1])
        return self.ws[o: o + n * self.dims[l + 1]].view(n, self.dims[l + 1])

    def run(self, x, ldx, n, y, y_off, ldy, route, npw=0):
        """Rows [0, n) of x (row pitch ldx; "composed": a multiple of 4 with zero pad columns) -> columns [y_off, y_off + width)
        of rows [0, n) of y (row pitch ldy)."""
        if not 1 <= n <= self.R:
            raise ValueError(f"{n} rows for a chain of at most {self.R}")
        base = self._params()
        if route == "rows":
            Ac, dg = self.policy or (0, False)
            call("tacorl_rows_mlp_fwd", ptr(x), ldx, len(self.acts), self._c_dims, self._w, self._b, self._c_acts, ptr(self.ws),
                 ops._at(y, y_off), ldy, n, int(self.policy is not None), Ac, int(dg), int(npw), ops.stream())
            return
        if route != "composed":
            raise ValueError(f"route {route!r}")
        if n not in self._yoff:
            self._yoff[n] = ops.mlp_act_layout(n, self.dims, self.acts)[1][-1]
        yo = self._yoff[n]
        ops.mlp_fwd([x], ldx, [base], [self.act], [n], self.dims, self.acts, F32)
        if self.policy is None:
            ops.copy_cols(self.act, yo, self.dims[-1], y, y_off, ldy, n, self.dims[-1])
        else:
            Ac, dg = self.policy
            ops.tanh_normal_sample(self.act[yo:], self.dims[-1], self.eps, self.gu, False, y, y_off, ldy, self.logp, self.grip,
                                   1, n, Ac)


def attach_ril_rollout_surface(module, engine):
    """RelayImitationLearning's rollout methods under the reference's names (evaluation/rollout_manager.py:434-557):
    `perceptual_encoder.get_state_from_observation`, a callable `goal_encoder`, and on `high_level_policy` /
    `low_level_policy` `get_actions`, `get_dist`, `action_dim`, `discrete_gripper`."""
    union = [c for c in engine.cams]
    shared = RILNetView(engine)
    runner = EncoderRunner(module)
    module.__dict__["_pe_runner"] = runner
    module.perceptual_encoder.get_state_from_observation = (
        lambda observation, modalities=None, cat_output=True: state_from_observation(
            module, runner, shared, observation, list(modalities if modalities is not None else union), cat_output))
    attach_goal_encoder(module, shared)
    module.__dict__["_rollout_nets"] = {"goal_encoder": shared}
    for key in ("high", "low"):
        net = RILNetView(engine, key)
        surf = ActorSurface(module, net, engine.order[key], engine.order[key], net.A, net.dg)
        box = getattr(module, key + "_level_policy")
        box.get_actions = surf.get_actions
        box.get_dist = PlanProposalSurface(module, net, net.Ac).get_dist
        box.action_dim, box.discrete_gripper = net.A, net.dg
        module.__dict__["_rollout_nets"][key] = net
