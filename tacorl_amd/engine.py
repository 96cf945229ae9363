"""Hand-scheduled actor-critic update (CQL_Offline.compute_update) on HIP kernels.

One `ACEngine.update()` = the reference's `compute_update`
(reference modules/cql/cql_offline_lightning.py:470-542) with the same loss values,
gradients, optimiser steps and soft target update, but scheduled MI355X-first:

* every unique (encoder, image set) is encoded once (11*B images instead of the reference's
  (24+12n)*B): the sample expansion `expand_obs` happens on 64-float embeddings;
* the five networks (actor, q1, q2, target_q1, target_q2) share launches through problem
  batches; every buffer is pre-allocated so the whole update is hipGraph-capturable;
* no autograd: forward and backward are explicit kernel sequences; parameters, gradients,
  Adam moments and targets are flat blocks (clip+Adam+Polyak = 2 launches per network).

Random draws are explicit inputs (`noise` dict, reference draw order - SURVEY 8a note 1).
"""
import torch

from . import blocks, ops
from . import encoder_stage as stage
from . import image_ingest as ingest
from . import dist as D
from . import noise as noise_mod
from ._lib import ACT_NONE, ACT_RELU, ACT_SILU, BF16, DR3_SLOTS, F32, LOG_SLOTS, call, ptr


def _al4(x):
    return (x + 3) // 4 * 4


class NetBlock:
    """[encoder(cam) for cam in cams] + goal-encoder MLP + head MLP in one flat buffer."""

    def __init__(self, cams, goal_cams, head_dims, head_acts, head_names, device, head_parts=None, hidden=256):
        self.cams, self.goal_cams = list(cams), list(goal_cams)
        self.all_cams = sorted(set(self.cams) | set(self.goal_cams))
        self.E_obs, self.G = 32 * len(self.cams), 32 * len(self.goal_cams)
        self.genc_dims, self.genc_acts = [self.G, hidden, hidden, self.G], [ACT_RELU, ACT_RELU, ACT_NONE]
        self.head_dims, self.head_acts = list(head_dims), list(head_acts)
        off = 0
        self.enc_off = {}
        for c in self.all_cams:
            self.enc_off[c] = off
            off += blocks.encoder_size()
        self.genc_off = off
        off += blocks.mlp_size(self.genc_dims)
        self.head_off = off
        off += blocks.mlp_size(self.head_dims)
        self.size = off
        self._head_names, self._head_parts = head_names, head_parts
        self._alloc_block(device)

    def _alloc_block(self, device):
        z = lambda: torch.zeros(self.size, device=device)  # noqa: E731
        self.param, self.grad, self.m, self.v = z(), z(), z(), z()
        # bf16 copy of the MLP part of the block (the fused MLP forward's MFMA operand); refreshed from
        # the fp32 master at the start of every update (ACEngine._refresh_bf16)
        self.param_bf16 = torch.zeros(self.size, device=device, dtype=torch.bfloat16)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.views, self.grad_views = self._views_of(self.param), self._views_of(self.grad)

    def _views_of(self, flat):
        """Reference-named views (logical shapes) into a flat block of this layout."""
        dst = {}
        for c in self.all_cams:
            for k, v in blocks.encoder_views(flat, self.enc_off[c]).items():
                dst[f"encoder.networks.{c}.{k}"] = v
        gn = [(f"goal_encoder.mlp.{i}.weight", f"goal_encoder.mlp.{i}.bias") for i in (0, 2, 4)]
        dst.update(blocks.mlp_views(flat, self.genc_off, self.genc_dims, gn))
        dst.update(self._head_views(flat))
        return dst

    def _head_views(self, flat):
        if self._head_parts is None:
            return blocks.mlp_views(flat, self.head_off, self.head_dims, self._head_names)
        dst = blocks.mlp_views(flat, self.head_off, self.head_dims[:-1], self._head_names)
        dst.update(blocks.head_views(flat, self.head_off, self.head_dims, self.head_dims[-2], self._head_parts))
        return dst

    def views_of(self, flat):
        return self._views_of(flat)

    def rebind_grad(self, flat):
        """Move the gradient block into caller-provided storage (a slice of one arena, so that a single
        all-reduce covers several networks)."""
        assert flat.numel() == self.size and flat.is_contiguous()
        flat.copy_(self.grad)
        self.grad = flat
        self.grad_views = self._views_of(flat)

    def enc(self, cam, flat=None):
        flat = self.param if flat is None else flat
        return flat.data_ptr() + 4 * self.enc_off[cam]

    def genc(self, flat=None):
        return (self.param if flat is None else flat).data_ptr() + 4 * self.genc_off

    def head(self, flat=None):
        return (self.param if flat is None else flat).data_ptr() + 4 * self.head_off

    def genc_bf16(self):
        return self.param_bf16.data_ptr() + 2 * self.genc_off

    def head_bf16(self):
        return self.param_bf16.data_ptr() + 2 * self.head_off


class Scalar:
    def __init__(self, device, value=0.0):
        self.param = torch.full((1,), float(value), device=device)
        self.grad, self.m, self.v = (torch.zeros(1, device=device) for _ in range(3))
        self.step = torch.zeros(1, dtype=torch.int32, device=device)


class ACEngine:
    def __init__(self, cams, goal_cams, hw, action_dim, B, device, *, n=4, discount=0.99, tau=0.005, actor_lr=3e-4,
                 critic_lr=3e-4, deterministic_backup=False, reward_scale=1.0, clip_grad_val=1.0,
                 conservative_weight=1.0, lagrange_thresh=5.0, temp=1.0, with_lagrange=False,
                 discrete_gripper=False, target_entropy=-7.0, policy_layers=3, q_layers=3, hidden=256,
                 compute=F32, img_dtype=torch.float32, world_size=1, dr3_coefficient=None):
        if dr3_coefficient is not None and not dr3_coefficient > 0:
            raise ValueError(f"dr3_coefficient must be positive (or None: no DR3 term), got {dr3_coefficient!r}")
        self.dr3 = None if dr3_coefficient is None else float(dr3_coefficient)
        if not cams or not goal_cams:
            raise NotImplementedError("observation and goal modalities must both be non-empty (the reference's no-goal "
                                      "branch is not built)")
        if len(set(cams)) != len(cams) or len(set(goal_cams)) != len(goal_cams):
            raise ValueError(f"a modality is listed twice: obs {list(cams)}, goal {list(goal_cams)}")
        self.cams, self.hw = list(cams), dict(hw or {})
        # Two ordered camera lists (reference visual_actor_wrapper.py:41-62): the state embedding is the cameras of `cams`
        # in list order, the goal encoder's input the cameras of `goal_cams` in list order; every network owns an encoder
        # per camera of the union.  enc_cams: every camera the step encodes (the observation cameras first).
        self.goal_cams = list(goal_cams)
        self.enc_cams = self.cams + [c for c in self.goal_cams if c not in self.cams]
        self.img_dtype = img_dtype
        self.Eo, self.G = 32 * len(self.cams), 32 * len(self.goal_cams)
        self.E = self.Eo + self.G
        self.lds = self.E
        self._init_step(action_dim, B, device, n, dict(
            discount=discount, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr, deterministic_backup=deterministic_backup,
            reward_scale=reward_scale, clip=clip_grad_val, cons_w=conservative_weight, gap=lagrange_thresh, temp=temp,
            target_entropy=target_entropy), with_lagrange, discrete_gripper, policy_layers, q_layers, hidden, compute, world_size)

    def _init_step(self, action_dim, B, device, n, hp, with_lagrange, discrete_gripper, policy_layers, q_layers, hidden, compute,
                   world_size):
        """Everything of the constructor that does not depend on where the state rows come from (self.E, self.lds are set):
        hyper-parameters, the five networks, the two temperatures, the gradient arena, the first batch's buffers."""
        self.B, self.n, self.A = B, n, action_dim
        self.dev, self.compute = device, compute
        self.dg = bool(discrete_gripper)
        self.Ac = action_dim - 1 if self.dg else action_dim
        self.HD = 2 * self.Ac + (2 if self.dg else 0)
        self.hp = hp
        self.with_lagrange = with_lagrange
        self.world = world_size
        self.hidden = hidden
        self.ldq = _al4(self.E + action_dim)
        pol_dims = [self.E] + [hidden] * policy_layers + [self.HD]
        q_dims = [self.E + action_dim] + [hidden] * q_layers + [1]
        silu_p, silu_q = [ACT_SILU] * policy_layers + [ACT_NONE], [ACT_SILU] * q_layers + [ACT_NONE]
        ap, qp = self.name_prefix
        pn = [(f"{ap}policy.fc_layers.{i}.weight", f"{ap}policy.fc_layers.{i}.bias") for i in range(policy_layers)]
        parts = [(f"{ap}policy.fc_mean", self.Ac), (f"{ap}policy.fc_log_std", self.Ac)]
        if self.dg:
            parts.append((f"{ap}policy.gripper_action", 2))
        qn = [(f"{qp}Q.fc_layers.{i}.weight", f"{qp}Q.fc_layers.{i}.bias") for i in range(q_layers)]
        qn.append((f"{qp}Q.out.weight", f"{qp}Q.out.bias"))
        self.actor = self._net_block(pol_dims, silu_p, pn, parts)
        self.q1, self.q2, self.tq1, self.tq2 = (self._net_block(q_dims, silu_q, qn, None) for _ in range(4))
        self.log_alpha, self.log_alpha_prime = Scalar(device), Scalar(device)
        # one gradient arena [actor | q1 | q2 | log_alpha'] -> ONE all-reduce per step for the update
        # (plus the scalar one for log_alpha, which must be stepped before the actor loss)
        self.arena_extra = []
        self._bind_arena()
        self.extra_enc, self.packs, self._prepacked = [], stage.PackedWeights(device), False
        self.fp_src = {}  # camera -> {"next": address of a stage.SourceTable entry}: set by the step that owns the batch
        self.B = None
        if B:
            self.ensure_batch(B)

    # reference names of the policy / Q tensors inside a network's block (the visual wrappers' sub-module names)
    name_prefix = ("actor.", "critic.")
    # DR3 coefficient (reference cql_offline_lightning.py:424-437), None: no such term.  With one, each critic's encoder also
    # encodes the next observations (forward only: problems q1_nx / q2_nx) and phase_b (_dr3) adds the term's value to the
    # logged critic losses and its gradient to the critics' state gradients.
    dr3 = None

    def _net_block(self, head_dims, head_acts, head_names, head_parts):
        return NetBlock(self.cams, self.goal_cams, head_dims, head_acts, head_names, self.dev, head_parts=head_parts,
                        hidden=self.hidden)

    def _bind_arena(self):
        """[actor | q1 | q2 | log_alpha' | extra blocks...]: every gradient the step's second collective reduces, one
        allocation (the fine-tuned action decoder's block rides in the same all-reduce)."""
        blks = [self.actor, self.q1, self.q2]
        sizes = [b.size for b in blks] + [4] + [b.size for b in self.arena_extra]
        arena = torch.zeros(sum(sizes), device=self.dev)
        o = 0
        for blk in blks:
            blk.rebind_grad(arena[o: o + blk.size])
            o += blk.size
        old = self.log_alpha_prime.grad
        arena[o: o + 1].copy_(old.reshape(-1)[:1])
        self.log_alpha_prime.grad = arena[o: o + 1]
        o += 4
        for blk in self.arena_extra:
            blk.rebind_grad(arena[o: o + blk.size])
            o += blk.size
        self.grad_arena = arena

    def extend_arena(self, blk):
        """Put another trainable block's gradients (TACORL: the fine-tuned action decoder) into the arena."""
        if not any(b is blk for b in self.arena_extra):
            ops.note_alloc()
            self.arena_extra.append(blk)
            self._bind_arena()

    # ------------------------------------------------------------------ buffers
    def ensure_batch(self, B, hw=None):
        """(Re)allocate every batch-sized buffer; parameters and optimiser state are untouched."""
        hw = dict(hw) if hw is not None else self.hw
        if self.B != B or hw != self.hw:
            self.B, self.hw = B, hw
            self._alloc()

    def _alloc(self):
        ops.note_alloc()
        self._alloc_encoder_stage()
        self._alloc_chains()

    def _alloc_encoder_stage(self):
        """The stage in front of the chains: image slots, encoder outputs / activations, the goal encoders' buffers, and the
        rows it hands to the chains - the state rows S, the Q input rows XQ / XQpi / XT - with the gradients that come back."""
        B, dev = self.B, self.dev
        f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        # Image slots of a camera, in units of B images: [obs | goal | next] for a camera in both roles, [obs | next] for an
        # observation-only camera, [goal] for a goal-only one (images that no role uses are neither packed nor encoded).
        self.slot, self.cam_probs, self.erow, self.nbwd = {}, {}, {}, {}
        for c in self.enc_cams:
            names = [s_ for s_, used in (("obs", c in self.cams), ("goal", c in self.goal_cams), ("next", c in self.cams)) if used]
            sl = self.slot[c] = {s_: i for i, s_ in enumerate(names)}
            # encoder problems (key, net, first image row in X3, n images): each a run of adjacent slots.  Both roles:
            # actor(obs, goal), actor(next), q1 / q2 (obs, goal), targets (goal, next) = 11*B images; observation only:
            # actor(obs), actor(next), q1 / q2 (obs), targets (next) = 6*B; goal only: five networks (goal) = 5*B.
            want = [("a_og", self.actor, ("obs", "goal")), ("a_nx", self.actor, ("next",)), ("q1", self.q1, ("obs", "goal")),
                    ("q2", self.q2, ("obs", "goal")), ("tq1", self.tq1, ("goal", "next")), ("tq2", self.tq2, ("goal", "next"))]
            if self.dr3 is not None:
                # DR3: the critics' own encoders over the next observations, forward only like a_nx (2*B more images per
                # observation camera; a goal-only camera has no `next` slot and gets no problem).  Problems of their own: the
                # q1 / q2 problems' activation buffers are laid out for the nbwd images their backward walks.
                want += [("q1_nx", self.q1, ("next",)), ("q2_nx", self.q2, ("next",))]
            pr = []
            for k, net, roles in want:
                have = [s_ for s_ in roles if s_ in sl]
                if not have:
                    continue
                r0 = sl[have[0]]
                assert [sl[s_] for s_ in have] == list(range(r0, r0 + len(have)))
                pr.append((k, net, r0 * B, len(have) * B))
                self.erow[(k, c)] = {s_: (sl[s_] - r0) * B for s_ in have}  # first enc_out row of each role's images
            self.cam_probs[c] = pr
            self.nbwd[c] = (("obs" in sl) + ("goal" in sl)) * B  # images of a problem that has a backward (GRAD_PROBS)
        self.X3 = ingest.LazyImages({c: torch.zeros(len(self.slot[c]) * B, *self.hw[c], 3, device=dev, dtype=self.img_dtype) for c in self.enc_cams})
        # (the first camera's table - every camera's when the two lists name the same cameras)
        self.enc_probs = self.cam_probs[self.enc_cams[0]]
        nimg = {(k, c): n_ for c in self.enc_cams for k, _, _, n_ in self.cam_probs[c]}
        keys = [kc for k in ("a_og", "a_nx", "q1", "q2", "tq1", "tq2", "q1_nx", "q2_nx") for c in self.enc_cams if (kc := (k, c)) in nimg]
        self.enc_out = {kc: f(nimg[kc], 32) for kc in keys}
        self.enc_act = {kc: f(ops.encoder_act_layout(nimg[kc], *self.hw[kc[1]])[1]) for kc in keys}
        self.enc_dout = {(k, c): f(self.nbwd[c], 32) for k in ("a_og", "q1", "q2") for c in self.enc_cams}
        nets = [("a", self.actor), ("q1", self.q1), ("q2", self.q2), ("tq1", self.tq1), ("tq2", self.tq2)]
        self.nets = nets
        self.gin = {k: f(B, self.G) for k, _ in nets}
        self.gact = {k: f(ops.mlp_act_layout(B, net.genc_dims, net.genc_acts)[2]) for k, net in nets}
        self.g_yoff = ops.mlp_act_layout(B, self.actor.genc_dims, self.actor.genc_acts)[1][-1]
        self.S = {k: f(B, self.lds) for k in ("a", "a_nx", "q1", "q2", "tq1", "tq2")}
        self.dS = {k: f(B, self.lds) for k in ("a", "q1", "q2")}
        self.dgin = {k: f(B, self.G) for k in ("a", "q1", "q2")}
        R = (3 * self.n + 1) * B
        self.XQ = {k: f(R, self.ldq) for k in ("q1", "q2")}
        self.XQpi = {k: f(B, self.ldq) for k in ("q1", "q2")}
        self.XT = {k: f(B, self.ldq) for k in ("tq1", "tq2")}
        self.dXQ = {k: f(R, self.ldq) for k in ("q1", "q2")}
        if self.dr3 is not None:
            # the DR3 launch's operands per critic: [enc(obs) | enc(next)] over the observation cameras, (B, Eo) each
            self.dr3_in = {k: (f(B, self.Eo), f(B, self.Eo)) for k in ("q1", "q2")}

    def _alloc_chains(self):
        """Buffers of the policy and Q chains, the sampled actions, the losses and the step's noise: what the step needs
        whatever produced its state rows self.S / Q input rows self.XQ, self.XQpi, self.XT."""
        B, n, dev = self.B, self.n, self.dev
        f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        pd, pa = self.actor.head_dims, self.actor.head_acts
        self.pact = {k: f(ops.mlp_act_layout(B, pd, pa)[2]) for k in ("a", "a_nx")}
        self.p_yoff = ops.mlp_act_layout(B, pd, pa)[1][-1]
        R = (3 * n + 1) * B
        self.R = R
        self.acts_main, self.act_pi, self.act_next = f(R, self.A), f(B, self.A), f(B, self.A)
        self.logp_pi, self.logp_next = f(B), f(B)
        self.logp_cur, self.logp_nxt = f(n * B), f(n * B)
        self.grip_pi = torch.zeros(B, dtype=torch.int32, device=dev)
        qd, qa = self.q1.head_dims, self.q1.head_acts
        self.qact = {k: f(ops.mlp_act_layout(R, qd, qa)[2]) for k in ("q1", "q2")}
        self.qact_pi = {k: f(ops.mlp_act_layout(B, qd, qa)[2]) for k in ("q1", "q2")}
        self.qact_t = {k: f(ops.mlp_act_layout(B, qd, qa)[2]) for k in ("tq1", "tq2")}
        self.q_yoff_R = ops.mlp_act_layout(R, qd, qa)[1][-1]
        self.q_yoff_B = ops.mlp_act_layout(B, qd, qa)[1][-1]
        self.dq = {k: f(R) for k in ("q1", "q2")}
        self.dq_pi = {k: f(B) for k in ("q1", "q2")}
        self.dXQpi = {k: f(B, self.ldq) for k in ("q1", "q2")}
        self.d_head = f(B, self.HD)
        self.reward, self.done = f(B), f(B)
        # the data action IS rows [0, B) of the Q networks' action column block (no copy in front of the Q forward):
        # load_transition / TACORL's plan-recognition sample write it in place
        self.action = self.acts_main[:B]
        # all noise of a step in ONE flat buffer [normal | uniform]: two generator launches per step with torch's generator
        # (one per part), one tacorl_noise_fill launch with a device-noise seed (self._noise_table, built here)
        shapes = dict(eps_pi=(B, self.Ac), eps_next=(B, self.Ac), eps_cur=(n, B, self.Ac), eps_nxt=(n, B, self.Ac))
        shapes.update(getattr(self, "extra_normal", {}))  # e.g. TACORL's plan-recognition eps
        ushapes = dict(u_rand=(n * B, self.A))
        if self.dg:
            ushapes.update(g_pi=(B, 2), g_next=(B, 2), g_cur=(n, B, 2), g_nxt=(n, B, 2))
        import math
        n_normal = sum(_al4(math.prod(v)) for v in shapes.values())
        flat = self._noise_flat = f(n_normal + sum(_al4(math.prod(v)) for v in ushapes.values()))
        self._noise_normal, self._noise_uniform = flat[:n_normal], flat[n_normal:]
        views, entries, off = {}, [], 0
        for kind, sh in (("normal", shapes), ("uniform", ushapes)):
            for k, v in sh.items():
                views[k] = flat[off: off + math.prod(v)].view(*v)
                entries.append((k, kind, off, v))
                off += _al4(math.prod(v))
        self._noise_table = noise_mod.table_for(flat.numel(), entries, B)
        self.extra_noise = {k: views[k] for k in getattr(self, "extra_normal", {})}
        self.noise = {k: views[k] for k in ("eps_pi", "eps_next", "u_rand", "eps_cur", "eps_nxt")}
        if self.dg:
            self.noise.update({k: views[k] for k in ("g_pi", "g_next", "g_cur", "g_nxt")})
        self.logs = f(32)
        self.cql_ws = torch.empty(max(256, ops.L.lib().tacorl_cql_ws_bytes(B)), dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------- inputs
    device_noise = None  # a noise.DeviceNoise: the step's noise from the counter-based generator (ModuleMixin.set_device_noise)

    def set_noise(self, noise=None):
        """Copy injected noise; or, with a device-noise seed (self.device_noise), fill every buffer for this rank's samples of
        the current step in one launch and advance the step; or draw with torch's device generator (two launches)."""
        if noise is None and self.device_noise is not None:
            self.device_noise.fill(self._noise_table, self._noise_flat, None, noise_mod.rank_sample0(self.B, self.world))
            self.device_noise.advance()
            return
        if noise is None:
            self._noise_normal.normal_()
            self._noise_uniform.uniform_()
            return
        for k, buf in self.noise.items():
            buf.copy_(noise[k].reshape(buf.shape))
        for k, buf in self.extra_noise.items():
            if k in noise:
                buf.copy_(noise[k].reshape(buf.shape))

    def load_images(self, cam, obs, goal, nxt, nchw=True):
        """obs/goal/nxt: (B,3,H,W) [nchw] or (B,H,W,3) fp32 device tensors (may be strided views with a
        uniform image pitch, e.g. states[:,0]); the images of a role the camera does not have are not read (None)."""
        given = {"obs": obs, "goal": goal, "next": nxt}
        sl = self.slot[cam]
        self.X3.drop(cam)
        ingest.pack_slots(self.X3.raw(cam), list(sl.values()), self.B, self.hw[cam], [given[s_] for s_ in sl], nchw, self.img_dtype)

    def load_transition(self, action, reward, done):
        self.action.copy_(action.reshape(self.B, self.A).float())
        self.reward.copy_(reward.reshape(self.B).float())
        self.done.copy_(done.reshape(self.B).float())

    # ----------------------------------------------------------------- forward
    def _img_ptr(self, cam, first_row):
        H, W = self.hw[cam]
        x3 = self.X3.raw(cam)  # (as it stands: on TACORL's fp32 route the next observations' slot is filled only for a reader)
        return x3.data_ptr() + first_row * H * W * 3 * x3.element_size()

    # Every encoder problem of a camera goes through the fused single-launch kernel when it applies
    # (bf16 images + bf16 MFMA + a templated camera geometry); the ones a backward follows (GRAD_PROBS)
    # also get their activations saved by that launch.  Otherwise: the per-layer path.
    GRAD_PROBS = ("a_og", "q1", "q2")
    use_fused = True  # tests flip this to compare the fused launch against the per-layer path
    EF_SPLIT_BUDGET = 160  # workgroups of the update's own encoder launch in encode_split

    def _fused_ok(self, c):
        return self.use_fused and stage.fused_fwd_ok(self.hw[c], self.compute, self.img_dtype)

    def _fused_bwd_ok(self, c):
        return self.use_fused and stage.fused_bwd_ok(self.hw[c], self.compute, self.img_dtype, [self.nbwd[c]] * 3)

    def _fused_saves(self, c):
        return self.use_fused and stage.fused_saves(self.hw[c], self.compute, self.img_dtype, [self.nbwd[c]] * 3)

    def _all_problems(self, c, which="all"):
        """(image pointer, net, out, act, n_img, needs_backward, camera) of every encoder problem of camera c
        (which = "own": the update's networks only, "extra": the caller's frozen ones only - TACORL's LMP window)."""
        pr, B = [], self.B
        nxt = self.fp_src.get(c, {}).get("next")  # the next observations as an fp32 source (TACORL's eligible batches)
        for k, net, r0, n in ([] if which == "extra" else self.cam_probs[c]):
            rows = self.erow[(k, c)]
            if nxt is None or "next" not in rows or k in self.GRAD_PROBS:
                pr.append((self._img_ptr(c, r0), net, self.enc_out[(k, c)], self.enc_act[(k, c)], n, k in self.GRAD_PROBS, c))
                continue
            # a forward-only problem over the next observations: their slot of X3 is not packed on this route - one problem
            # per role, the next observations read from where the batch lies, the others from their packed slots
            for role, row in rows.items():
                pr.append((self._img_ptr(c, self.slot[c][role] * B), net, self.enc_out[(k, c)][row: row + B], self.enc_act[(k, c)],
                           B, False, c, nxt if role == "next" else None))
        if which != "own":
            pr += [(x["img"], x["net"], x["out"], x["act"], x["n"], False, c, x.get("src")) for x in self.extra_enc if x["cam"] == c]
        return pr

    def encode_split(self, between):
        """(Fused path only): the frozen extra problems (TACORL: the LMP window, whose embeddings the plan recognition ->
        action decoder branch waits for) as a launch of their own FIRST, `between()` (the caller forks that branch there),
        then the update's own problems on EF_SPLIT_BUDGET workgroups (160: 96 CUs stay free for the branch; sweep 96 .. 240
        on C4 / C3: 128 - 160 best).  Returns False when the split does not apply (nothing launched)."""
        groups = self._fused_groups()
        if not self.extra_enc or len(groups) != 1 or sorted(groups[0]) != sorted(self.enc_cams) or not all(self._fused_bwd_ok(c) for c in self.enc_cams):
            return False
        self._encode(groups, "extra")
        between()
        self._encode(groups, "own", max_wg=self.EF_SPLIT_BUDGET)
        return True

    # The packed conv weights of the fused forward (stage.PackedWeights states the rule): the five networks the optimiser
    # moves are packed BEHIND the Adam launch (phase_c) - in the shadow of the action-decoder branch, which ends later -
    # and the frozen extra networks (TACORL's LMP encoder) once, in front of the first forward that reads them.
    def _late_pack_nets(self):
        return [self.actor, self.q1, self.q2, self.tq1, self.tq2]

    def packs_stale(self):
        """(Every network of the step's encoder launch: the optimiser's ones AND the extra, frozen ones.)"""
        return self.packs.stale(self._late_pack_nets() + [x["net"] for x in self.extra_enc], self.enc_cams)

    def packs_written(self):
        self.packs.written(self._late_pack_nets(), self.enc_cams)

    def _launch_fused(self, c, pr, max_wg=0):
        """One fused encoder launch over the problems pr, cameras of camera c's geometry (bench.py times the step's fused
        launches by replacing this method on the instance)."""
        stage.launch_fused(pr, self.packs, self.hw[c], max_wg)

    def _fused_groups(self):
        """Cameras whose fused encoder problems share ONE launch (stage.geometry_groups); cameras without the fused forward
        are in no group."""
        return [cs for cs in self._camera_groups(stage.EF_MAXP, lambda c: len(self._all_problems(c))) if self._fused_ok(cs[0])]

    def _camera_groups(self, limit, n_problems):
        return stage.geometry_groups(self.enc_cams, self.hw, self._fused_bwd_ok, n_problems, limit)

    def encode_fused_only(self):
        """Just the fused encoder launch(es) of the step (bench roofline probe).  Returns images per step."""
        n_total = 0
        for cs in self._fused_groups():
            pr = [x for c in cs for x in self._all_problems(c)]
            self._launch_fused(cs[0], pr)
            n_total += sum(x[4] for x in pr)
        return n_total

    def _encode(self, groups, which, max_wg=0):
        stage.encode(groups, lambda c: self._all_problems(c, which), self.hw, self.compute, self.img_dtype, self.packs,
                     self._fused_ok, self._fused_saves, lambda c, pr: self._launch_fused(c, pr, max_wg))

    def _encode_all(self):
        """Every encoder forward of the step: ONE fused launch per camera group (27*B images at TACORL shapes:
        frozen LMP window, actor(obs, goal, next), q1, q2 and both targets), activations saved only for the
        problems that have a backward; the per-layer path covers fp32 mode / images too large for LDS."""
        self._encode(self._camera_groups(stage.EF_MAXP, lambda c: len(self._all_problems(c))), "all")

    def _refresh_bf16(self):
        """bf16 copies of the five networks' MLP weights, the fused MLP kernels' MFMA operand (one launch, every step); the
        fp32 blocks stay the masters.  Having the Adam / Polyak launch write them instead measured slower (round 5, ms/step:
        0.8370 with this launch against 0.8431 - 0.8485 without): the few microseconds by which it delays phase_a's first MLP
        launch let the plan recognition's 256 one-per-CU workgroups all start at once, and the action-decoder branch behind
        them - the step's co-critical chain - starts that much earlier."""
        if self.compute != BF16:
            return
        nets = [self.actor, self.q1, self.q2, self.tq1, self.tq2]
        call("tacorl_to_bf16_batch", len(nets), ops.ptr_array([n_.genc() for n_ in nets]),
             ops.ptr_array([n_.genc_bf16() for n_ in nets]), (ops.C.c_long * len(nets))(*[n_.size - n_.genc_off for n_ in nets]),
             ops.stream())

    def _mlp_bwd_sites(self):
        """(tag, params, M, dims) of every fused-MLP backward of the update, as _mlp_backward receives them."""
        B = self.B
        qd, pd, gd = self.q1.head_dims, self.actor.head_dims, self.actor.genc_dims
        return [("q", [self.q1.head(), self.q2.head()], [self.R, self.R], qd),
                ("qpi", [self.q1.head(), self.q2.head()], [B, B], qd),
                ("pi", [self.actor.head()], [B], pd),
                ("genc", [self.actor.genc(), self.q1.genc(), self.q2.genc()], [B] * 3, gd)]

    def _prepack_backward(self):
        """Weight-only preparation of the backward kernels (transposed MLP weights, conv W^T fragments) in front of the
        forward: six small launches that would otherwise sit on the dependent chain of the backward.  In line (round 5): they
        are small enough in registers to run beside the plan recognition's workgroups, which the fused MLP forwards that
        follow are not, and on a side branch of the graph the fork / join made the step 8 us longer."""
        self._prepacked = False
        if self.compute != BF16:
            return
        for tag, params, M, dims in self._mlp_bwd_sites():
            ops.mlp_bwd_fused_pack(params, M, dims, "mlp_bwdf_" + tag, self.dev)
        nets = [self.actor, self.q1, self.q2]
        for cs in self._ebw_sequences():
            ws, n3 = self._ebw_workspace(cs)
            if ws is not None:
                H, W = self.hw[cs[0]]
                call("tacorl_encoder_bwd_fused_pack", len(n3), ops.ptr_array([x.enc(cc) for cc in cs for x in nets]), ops.int_array(n3),
                     H, W, ptr(ws), ws.numel(), ops.stream())
        self._prepacked = True

    # Gathered MLP inputs (round 5): the concatenations in front of the goal encoders, the policy head and the Q heads are
    # read by the fused forward's input stage where their producers left them (ops.mlp_fwd_gather) instead of being
    # assembled by a copy launch first - three launches fewer on the step's dependent chain.  A shape the gathered forward
    # does not take (f32 mode, C5's many-row Q problems) goes through copy + forward.
    def _gather_ok(self, tag):
        if self.compute != BF16:
            return False
        cache = self.__dict__.setdefault("_gather_cache", {})
        key = (tag, self.B)
        if key not in cache:
            B = self.B
            M, net, ldx = {"genc": ([B] * 5, (self.actor.genc_dims, self.actor.genc_acts), self.G),
                           "pi": ([B] * 2, (self.actor.head_dims, self.actor.head_acts), self.lds),
                           "q": ([self.R, self.R, B, B, B, B], (self.q1.head_dims, self.q1.head_acts), self.ldq)}[tag]
            # (segment pitches must be multiples of 4 floats: the action block's is A - 7 for the CQL baseline; every
            # segment starts on a multiple of 8 columns at a 16-byte aligned address - mlp_set_gather's conditions, checked
            # here so that a geometry outside them takes the copy + forward path instead of failing inside the step)
            geom_ok = self.G % 4 == 0 and self.Eo % 8 == 0 and self.E % 8 == 0 and self.g_yoff % 4 == 0
            cache[key] = geom_ok and (tag != "q" or self.A % 4 == 0) and ops.mlp_fwd_gather_ok(
                M, net[0], net[1], ldx, self.compute, self._lean(tag))
        return cache[key]

    def _emb_segs(self, ek, role, gk, mod=0):
        """[enc(obs or next) per observation camera | goal_enc(enc(goal))] as input segments."""
        segs = [(self.enc_out[(ek, c)], self.erow[(ek, c)][role] * 32, 32, 32 * j, mod) for j, c in enumerate(self.cams)]
        segs.append((self.gact[gk], self.g_yoff, self.G, self.Eo, mod))
        return segs

    def _goal_rows(self, ek, c):
        """First float of camera c's goal embeddings in the encoder problem ek's output."""
        return self.erow[(ek, c)]["goal"] * 32

    # (encoder problem, role of the state images, goal-encoder net)
    _OBS_SRC = {"a": ("a_og", "obs", "a"), "a_nx": ("a_nx", "next", "a"), "q1": ("q1", "obs", "q1"), "q2": ("q2", "obs", "q2"),
                "tq1": ("tq1", "next", "tq1"), "tq2": ("tq2", "next", "tq2")}

    def _assemble_states(self):
        B = self.B
        # goal-encoder inputs: concat over the goal cameras of enc(goal)
        src = {"a": "a_og", "q1": "q1", "q2": "q2", "tq1": "tq1", "tq2": "tq2"}
        nets = dict(self.nets)
        ks = ["a", "q1", "q2", "tq1", "tq2"]
        if self._gather_ok("genc"):
            segs = [[(self.enc_out[(src[k], c)], self._goal_rows(src[k], c), 32, 32 * j, 0) for j, c in enumerate(self.goal_cams)]
                    for k in ks]
            ops.mlp_fwd_gather(segs, [self.gin[k] for k in ks], self.G, [nets[k].genc() for k in ks],
                               [nets[k].genc_bf16() for k in ks], [self.gact[k] for k in ks], [B] * 5, self.actor.genc_dims,
                               self.actor.genc_acts, lean=self._lean("genc"))
        else:
            with ops.copy_batch():
                for k, ek in src.items():
                    for j, c in enumerate(self.goal_cams):
                        ops.copy_cols(self.enc_out[(ek, c)], self._goal_rows(ek, c), 32, self.gin[k], 32 * j, self.G, B, 32)
            ops.mlp_fwd([self.gin[k] for k in ks], self.G, [nets[k].genc() for k in ks], [self.gact[k] for k in ks],
                        [B] * 5, self.actor.genc_dims, self.actor.genc_acts, self.compute,
                        params_bf16=[nets[k].genc_bf16() for k in ks], lean=self._lean("genc"))
        # S = [enc(obs or next) | goal_enc(enc(goal))]: assembled by a copy only for the forwards that do not gather
        need = [k for k in self._OBS_SRC if not self._gather_ok("pi" if k in ("a", "a_nx") else "q")]
        if need:
            with ops.copy_batch():
                for k in need:
                    ek, role, gk = self._OBS_SRC[k]
                    for j, c in enumerate(self.cams):
                        ops.copy_cols(self.enc_out[(ek, c)], self.erow[(ek, c)][role] * 32, 32, self.S[k], 32 * j, self.lds, B, 32)
                    ops.copy_cols(self.gact[gk], self.g_yoff, self.G, self.S[k], self.Eo, self.lds, B, self.G)

    def _policy_fwd(self):
        ks = ["a", "a_nx"]
        if self._gather_ok("pi"):
            segs = [self._emb_segs(*self._OBS_SRC[k]) for k in ks]
            # (S["a"] is the policy head's layer-0 operand in the backward: written from the forward's registers)
            ops.mlp_fwd_gather(segs, [self.S["a"], None], self.lds, [self.actor.head()] * 2, [self.actor.head_bf16()] * 2,
                               [self.pact[k] for k in ks], [self.B] * 2, self.actor.head_dims, self.actor.head_acts,
                               lean=self._lean("pi"))
            return
        ops.mlp_fwd([self.S[k] for k in ks], self.lds, [self.actor.head()] * 2, [self.pact[k] for k in ks],
                    [self.B] * 2, self.actor.head_dims, self.actor.head_acts, self.compute,
                    params_bf16=[self.actor.head_bf16()] * 2, lean=self._lean("pi"))

    def _head(self, k):
        return self.pact[k][self.p_yoff: self.p_yoff + self.B * self.HD]

    def update(self, bc_phase, optimize=True, encoded=False):
        """One compute_update.  Inputs must have been staged with load_images / load_transition /
        set_noise.  Returns nothing; metrics are in self.logs (read with metrics()).
        encoded=True: the caller already ran _encode_all() for this batch.

        Three collective-free phases (each hipGraph-capturable) separated by the step's two all-reduces:
        a) forward up to the alpha gradient; b) alpha step, critics, losses, every backward;
        c) optimiser steps + soft target update."""
        self.phase_a(encoded, optimize)
        self.allreduce_alpha()
        self.phase_b(bc_phase, optimize)
        self.allreduce_grads()
        self.phase_c(optimize)

    def allreduce_alpha(self):
        self._allreduce([self.log_alpha.grad])

    def allreduce_grads(self):
        self._allreduce([self.grad_arena])

    def phase_a(self, encoded=False, optimize=True):
        B, n, A, Ac, hp, nz = self.B, self.n, self.A, self.Ac, self.hp, self.noise
        gs = 1.0 / self.world
        if not encoded:
            self._encode_all()
        ops.mark("a:start")
        # (round 5: the weight-only launches of the two calls below - bf16 mirrors, transposed weights of the four MLP backward
        # sites and of the encoders' FC tails: 7 launches of 5 - 7 us on this chain - leave as ONE, ops.prep_batch)
        with ops.prep_batch():
            self._refresh_bf16()
            self._prepack_backward()
        self._assemble_states()
        self._policy_fwd()
        ops.mark("a:policy_fwd")
        head_cur, head_next = self._head("a"), self._head("a_nx")
        g = (lambda k: nz[k]) if self.dg else (lambda k: None)
        # one launch: rsample on obs, critic-target sample on next_obs, the n CQL samples on both, uniform actions
        at = ops._at
        jobs = [(head_cur, nz["eps_pi"], g("g_pi"), 1, ptr(self.act_pi), self.logp_pi, self.grip_pi if self.dg else None, 1),
                (head_next, nz["eps_next"], g("g_next"), 0, ptr(self.act_next), self.logp_next, None, 1),
                (head_cur, nz["eps_cur"], g("g_cur"), 0, at(self.acts_main, (1 + n) * B * A), self.logp_cur, None, n),
                (head_next, nz["eps_nxt"], g("g_nxt"), 0, at(self.acts_main, (1 + 2 * n) * B * A), self.logp_nxt, None, n)]
        call("tacorl_tanh_normal_sample_batch", len(jobs), ops.ptr_array([j[0] for j in jobs]), self.HD,
             ops.ptr_array([j[1] for j in jobs]), ops.ptr_array([j[2] for j in jobs]), ops.int_array([j[3] for j in jobs]),
             ops.ptr_array([j[4] for j in jobs]), A, ops.ptr_array([j[5] for j in jobs]),
             ops.ptr_array([j[6] for j in jobs]), ops.int_array([j[7] for j in jobs]), B, Ac, ptr(nz["u_rand"]),
             at(self.acts_main, B * A), n * B, A, int(self.dg), ops.stream())
        # alpha: loss, gradient, Adam step (alpha is read post-step below; SURVEY 8a note 2)
        # (one GPU and an optimising step: loss + gradient + Adam in one launch; otherwise the step follows collective #1)
        self._alpha_stepped = bool(optimize and not D.collectives_on(self.world) and not getattr(self, "split_alpha_step", False))
        if self._alpha_stepped:
            la = self.log_alpha
            call("tacorl_alpha_loss_step", ptr(self.logp_pi), B, ptr(la.param), float(hp["target_entropy"]), ptr(la.grad),
                 ptr(self.logs), ptr(la.m), ptr(la.v), float(hp["actor_lr"]), ptr(la.step), ops.stream())
        else:
            call("tacorl_alpha_loss", ptr(self.logp_pi), B, ptr(self.log_alpha.param), float(hp["target_entropy"]), gs,
                 ptr(self.log_alpha.grad), ptr(self.logs), ops.stream())
        ops.mark("a:alpha")
        ops.mark("a:end")

    def phase_b(self, bc_phase, optimize=True):
        B, n, A, Ac, hp, nz = self.B, self.n, self.A, self.Ac, self.hp, self.noise
        gs = 1.0 / self.world
        head_cur = self._head("a")
        if optimize and not getattr(self, "_alpha_stepped", False):
            ops.adam_step(self.log_alpha.param, self.log_alpha.grad, self.log_alpha.m, self.log_alpha.v,
                          hp["actor_lr"], 0.0, self.log_alpha.step)
        # Q inputs: [S | action]; the data action is read here first (phase_a does not need it, so a caller
        # may still be producing it - TACORL's plan recognition runs beside phase_a): wait for it if asked
        if getattr(self, "action_ready", None) is not None:
            torch.cuda.current_stream().wait_event(self.action_ready)
            self.action_ready = None
        ops.mark("b:start")
        self._q_forward()
        qout = lambda buf, off, rows: buf[off: off + rows]  # noqa: E731
        q1m, q2m = qout(self.qact["q1"], self.q_yoff_R, self.R), qout(self.qact["q2"], self.q_yoff_R, self.R)
        q1p, q2p = qout(self.qact_pi["q1"], self.q_yoff_B, B), qout(self.qact_pi["q2"], self.q_yoff_B, B)
        t1, t2 = qout(self.qact_t["tq1"], self.q_yoff_B, B), qout(self.qact_t["tq2"], self.q_yoff_B, B)
        # Bellman + CQL (+Lagrange): losses and dL/dq for every row
        lap = self.log_alpha_prime
        call("tacorl_cql_loss", ptr(q1m), ptr(q2m), ptr(self.dq["q1"]), ptr(self.dq["q2"]), ptr(t1), ptr(t2),
             ptr(self.logp_cur), ptr(self.logp_nxt), ptr(self.logp_next), ptr(self.reward), ptr(self.done),
             ptr(self.log_alpha.param), ptr(lap.param) if self.with_lagrange else None, B, n, A,
             float(hp["discount"]), float(hp["reward_scale"]), float(hp["temp"]), float(hp["cons_w"]),
             float(hp["gap"]), int(hp["deterministic_backup"]), gs, ptr(lap.grad), ptr(self.logs), ptr(self.cql_ws),
             self.cql_ws.numel(), ops.stream())
        ops.mark("b:q_fwd+cql")
        # ---- actor backward: independent of the critic backward until the goal encoders, so it runs on a
        # side stream (a parallel branch of the captured graph); both are chains of small launches that
        # fill only part of the chip on their own
        if getattr(self, "_bwd_stream", None) is None:
            self._bwd_stream = torch.cuda.Stream(device=self.dev)
        main_stream = torch.cuda.current_stream()
        self._bwd_stream.wait_stream(main_stream)
        # (round 5: the slab reduces behind the five one-launch weight gradients below - readers: all-reduce and optimiser -
        # are recorded and leave as ONE launch at the end of the phase, ops.reduce_batch)
        with ops.reduce_batch(auto=self.R >= 16384):
            with torch.cuda.stream(self._bwd_stream):
                self._actor_backward(bc_phase, head_cur, q1p, q2p, gs)
                ops.mark("b:actor_bwd")
            self._critic_backward()
            if self.dr3 is not None:
                self._dr3(gs)  # behind _state_grads_from_q (it ADDS into dS), in front of _encoders_backward (which reads dS)
            ops.mark("b:critic_bwd")
            main_stream.wait_stream(self._bwd_stream)
            self._encoders_backward()
            ops.mark("b:enc_bwd")
        ops.mark("b:end")

    def _q_forward(self):
        """The six Q forwards of the step (q1 / q2 over all R rows and over pi(obs), the targets over pi(next)), with the
        assembly of their input rows [S | action]."""
        B, A = self.B, self.A
        qd, qa = self.q1.head_dims, self.q1.head_acts
        ps = [self.q1.head(), self.q2.head(), self.q1.head(), self.q2.head(), self.tq1.head(), self.tq2.head()]
        ac = [self.qact["q1"], self.qact["q2"], self.qact_pi["q1"], self.qact_pi["q2"], self.qact_t["tq1"],
              self.qact_t["tq2"]]
        pb = [self.q1.head_bf16(), self.q2.head_bf16(), self.q1.head_bf16(), self.q2.head_bf16(), self.tq1.head_bf16(),
              self.tq2.head_bf16()]
        if self._gather_ok("q"):
            # Q inputs [enc(obs) | goal_enc | action] read in place: the state rows repeat every B rows (expand_obs on
            # embeddings), the actions are acts_main = [data | uniform | n x pi(obs) | n x pi(next)]; only the two
            # problems with weight gradients (q1 / q2 over all R rows) also write their assembled rows
            E = self.E
            seg = lambda k, mod, a_t: self._emb_segs(*self._OBS_SRC[k], mod) + [(a_t, 0, A, E, 0)]  # noqa: E731
            segs = [seg("q1", B, self.acts_main), seg("q2", B, self.acts_main), seg("q1", 0, self.act_pi), seg("q2", 0, self.act_pi),
                    seg("tq1", 0, self.act_next), seg("tq2", 0, self.act_next)]
            # (the q1 / q2 rows also as the bf16 operand of their weight gradients, where the backward site keeps one -
            # thousands of rows -: the forward holds those chunks in registers, the conversion was a launch of the critic backward)
            xb = self._q_xb()
            self._q_xb_current = all(x is not None for x in xb)
            ops.mlp_fwd_gather(segs, [self.XQ["q1"], self.XQ["q2"], None, None, None, None], self.ldq, ps, pb, ac,
                               [self.R, self.R, B, B, B, B], qd, qa, lean=self._lean("q"),
                               xb_out=xb + [None] * 4 if self._q_xb_current else None)
        else:
            self._q_xb_current = False
            self._assemble_q_rows()
            xs = [self.XQ["q1"], self.XQ["q2"], self.XQpi["q1"], self.XQpi["q2"], self.XT["tq1"], self.XT["tq2"]]
            ops.mlp_fwd(xs, self.ldq, ps, ac, [self.R, self.R, B, B, B, B], qd, qa, self.compute, params_bf16=pb, lean=self._lean("q"))

    def _q_xb(self):
        """Where the q1 / q2 problems' bf16 input rows lie in the Q backward site's workspace ([None] where it keeps none);
        looked up again only when a buffer has been (re)allocated."""
        key = (ops.alloc_epoch(), self.R)
        if getattr(self, "_q_xb_cache", (None,))[0] != key:
            ok = self._lean("q") and self.R < 16384
            xb = ops.mlp_bwd_fused_xb([self.R, self.R], self.q1.head_dims, "mlp_bwdf_q", self.dev) if ok else [None]
            self._q_xb_cache = ((ops.alloc_epoch(), self.R), xb)  # (the lookup itself may allocate the workspace)
        return self._q_xb_cache[1]

    def _assemble_q_rows(self):
        """XQ / XQpi / XT = [S | action] for the forwards that do not gather (one launch)."""
        B, A = self.B, self.A
        with ops.copy_batch():
            for k in ("q1", "q2"):
                ops.copy_cols(self.S[k], 0, self.lds, self.XQ[k], 0, self.ldq, self.R, self.E, src_row_mod=B)
                ops.copy_cols(self.acts_main, 0, A, self.XQ[k], self.E, self.ldq, self.R, A)
                ops.copy_cols(self.S[k], 0, self.lds, self.XQpi[k], 0, self.ldq, B, self.E)
                ops.copy_cols(self.act_pi, 0, A, self.XQpi[k], self.E, self.ldq, B, A)
            for k in ("tq1", "tq2"):
                ops.copy_cols(self.S[k], 0, self.lds, self.XT[k], 0, self.ldq, B, self.E)
                ops.copy_cols(self.act_next, 0, A, self.XT[k], self.E, self.ldq, B, A)

    def _critic_backward(self):
        """Critic backward through the Q MLPs; sum the broadcast embedding gradient over samples."""
        qd, qa = self.q1.head_dims, self.q1.head_acts
        self._mlp_backward("q", [self.XQ["q1"], self.XQ["q2"]], self.ldq, [self.q1.head(), self.q2.head()],
                           [self.qact["q1"], self.qact["q2"]], [self.dq["q1"], self.dq["q2"]], 1,
                           [self.q1.head(self.q1.grad), self.q2.head(self.q2.grad)], [self.dXQ["q1"], self.dXQ["q2"]],
                           self.ldq, [self.R, self.R], qd, qa, xb_current=self._q_xb_current)
        self._state_grads_from_q()

    def _state_grads_from_q(self):
        B, n = self.B, self.n
        call("tacorl_reduce_rows_mod_batch", 2, ops.ptr_array([self.dXQ["q1"], self.dXQ["q2"]]), self.ldq,
             ops.ptr_array([self.dS["q1"], self.dS["q2"]]), self.lds, B, self.E, 3 * n + 1, ops.stream())

    def _dr3(self, gs):
        """q{1,2}_dr3_loss = dr3 * mean_b <enc_qk(obs)[b], enc_qk(next)[b]> over the observation cameras, enc(next) a constant
        (reference cql_offline_lightning.py:424-437): two launches on the main stream, nodes of the captured step like their
        neighbours.  The encoders' fp32 outputs of both image sets are gathered camera by camera, in the order of `cams`,
        into (B, Eo) rows (one copy launch: the fused forwards may read the embeddings in place, so S is not always
        assembled); then ONE launch for both critics logs the term, adds it to q{1,2}_loss (tacorl_cql_loss has written
        them on this stream) and adds dr3 * gs / B * enc(next) into the observation columns of dS - the only gradient of
        the term, which the encoder backward then carries into the critics' encoders."""
        B, ks = self.B, ("q1", "q2")
        with ops.copy_batch():
            for k in ks:
                for j, c in enumerate(self.cams):
                    ops.copy_cols(self.enc_out[(k, c)], self.erow[(k, c)]["obs"] * 32, 32, self.dr3_in[k][0], 32 * j, self.Eo, B, 32)
                    ops.copy_cols(self.enc_out[(k + "_nx", c)], self.erow[(k + "_nx", c)]["next"] * 32, 32, self.dr3_in[k][1],
                                  32 * j, self.Eo, B, 32)
        call("tacorl_dr3_fwd_bwd", 2, ops.ptr_array([self.dr3_in[k][0] for k in ks]), self.Eo,
             ops.ptr_array([self.dr3_in[k][1] for k in ks]), self.Eo, ops.ptr_array([self.dS[k] for k in ks]), self.lds, B, self.Eo,
             self.dr3, gs, ptr(self.logs), ops.int_array([LOG_SLOTS.index(k + "_dr3_loss") for k in ks]),
             ops.int_array([LOG_SLOTS.index(k + "_loss") for k in ks]), ops.stream())

    _q_xb_current = False  # set by _q_forward: it has written the Q weight gradients' bf16 input rows (_q_xb)
    lean_mlp_acts = True  # hidden-layer outputs of the fused MLPs are recomputed by the weight-gradient launch, not saved

    def _lean(self, tag):
        """True when the MLP site's forward may skip its hidden-layer outputs: its whole backward is the fused pair
        (input-gradient chain + one-launch weight gradients), the only reader of those outputs."""
        if self.compute != BF16 or not self.lean_mlp_acts:
            return False
        tag = {"qpi": "q"}.get(tag, tag)
        cache = self.__dict__.setdefault("_lean_cache", {})
        if tag not in cache:
            n, dims, ldx, ldo, ldd = {"genc": (5, self.actor.genc_dims, self.G, self.lds, self.G),
                                      "pi": (2, self.actor.head_dims, self.lds, self.HD, self.lds),
                                      "q": (6, self.q1.head_dims, self.ldq, 1, self.ldq)}[tag]
            cache[tag] = ops.mlp_lean_ok(n, dims, ldx, ldo, ldd, self.compute) and ops.mlp_bwd_fused_ok(n, dims, ldo, ldd, self.compute)
        return cache[tag]

    def _mlp_backward(self, tag, *sites, **kw):
        ops.mlp_backward(("mlp_bwd_" + tag, "mlp_bwdf_" + tag), *sites, self.compute, prepacked=self._prepacked, lean=self._lean(tag),
                         **kw)

    def _actor_backward(self, bc_phase, head_cur, q1p, q2p, gs):
        B, A, Ac, nz = self.B, self.A, self.Ac, self.noise
        qd, qa = self.q1.head_dims, self.q1.head_acts
        if bc_phase:
            call("tacorl_actor_head_bwd", ptr(head_cur), self.HD, ptr(nz["eps_pi"]), ptr(self.logp_pi), None, None, 0,
                 ptr(self.action), A, ptr(self.grip_pi) if self.dg else None, ptr(self.log_alpha.param), gs,
                 ptr(self.d_head), B, Ac, int(self.dg), ptr(self.logs), ops.stream())
        else:
            call("tacorl_actor_qmin", ptr(q1p), ptr(q2p), ptr(self.logp_pi), B, ptr(self.log_alpha.param),
                 ptr(self.dq_pi["q1"]), ptr(self.dq_pi["q2"]), gs, ptr(self.logs), ops.stream())
            self._mlp_backward("qpi", [self.XQpi["q1"], self.XQpi["q2"]], self.ldq, [self.q1.head(), self.q2.head()],
                               [self.qact_pi["q1"], self.qact_pi["q2"]], [self.dq_pi["q1"], self.dq_pi["q2"]], 1,
                               [None, None], [self.dXQpi["q1"], self.dXQpi["q2"]], self.ldq, [B, B], qd, qa)
            call("tacorl_actor_head_bwd", ptr(head_cur), self.HD, ptr(nz["eps_pi"]), ptr(self.logp_pi),
                 ops._at(self.dXQpi["q1"], self.E), ops._at(self.dXQpi["q2"], self.E), self.ldq, None, 0,
                 ptr(self.grip_pi) if self.dg else None, ptr(self.log_alpha.param), gs, ptr(self.d_head), B, Ac,
                 int(self.dg), ptr(self.logs), ops.stream())
        self._mlp_backward("pi", [self.S["a"]], self.lds, [self.actor.head()], [self.pact["a"]], [self.d_head], self.HD,
                           [self.actor.head(self.actor.grad)], [self.dS["a"]], self.lds, [B], self.actor.head_dims,
                           self.actor.head_acts)

    def _ebw_sequences(self):
        """Camera groups that share one conv-backward launch sequence (3 networks per camera; C4: both cameras 128 x 128 -> one
        6-problem sequence instead of two 3-problem ones)."""
        return self._camera_groups(stage.EBW_MAXP, lambda c: 3)

    def _ebw_workspace(self, cs):
        """(scratch buffer of the group's fused backward - None where it takes the per-layer path -, images per problem)"""
        n3 = [self.nbwd[cc] for cc in cs for _ in range(3)]
        if not self._fused_bwd_ok(cs[0]):
            return None, n3
        return ops.encoder_bwd_fused_workspace(n3, *self.hw[cs[0]], self.dev, "enc_bwd_fused_" + "+".join(cs)), n3

    def _encoders_backward(self):
        """Goal encoders (3 nets, one batch), then the three encoders (actor(obs, goal), q1, q2)."""
        B = self.B
        nets = {"a": self.actor, "q1": self.q1, "q2": self.q2}
        ks = ["a", "q1", "q2"]
        self._mlp_backward("genc", [self.gin[k] for k in ks], self.G, [nets[k].genc() for k in ks],
                           [self.gact[k] for k in ks], [ops._at(self.dS[k], self.Eo) for k in ks], self.lds,
                           [nets[k].genc(nets[k].grad) for k in ks], [self.dgin[k] for k in ks], self.G, [B] * 3,
                           self.actor.genc_dims, self.actor.genc_acts)
        ek = {"a": "a_og", "q1": "q1", "q2": "q2"}
        with ops.copy_batch():
            # an observation camera's columns of dS are its index in `cams`, a goal camera's columns of dgin its index in
            # `goal_cams`; a camera in both roles gets both (its weight gradients sum over the 2*B images)
            for c in self.enc_cams:
                for k in ks:
                    rows = self.erow[(ek[k], c)]
                    if "obs" in rows:
                        ops.copy_cols(self.dS[k], 32 * self.cams.index(c), self.lds, self.enc_dout[(ek[k], c)], rows["obs"] * 32, 32, B, 32)
                    if "goal" in rows:
                        ops.copy_cols(self.dgin[k], 32 * self.goal_cams.index(c), self.G, self.enc_dout[(ek[k], c)], rows["goal"] * 32,
                                      32, B, 32)
        for cs in self._ebw_sequences():
            H, W = self.hw[cs[0]]
            pairs = [(nets[k], ek[k], cc) for cc in cs for k in ks]
            imgs = [self._img_ptr(cc, 0) for _, _, cc in pairs]
            acts, douts = [self.enc_act[(e_, cc)] for _, e_, cc in pairs], [self.enc_dout[(e_, cc)] for _, e_, cc in pairs]
            params, grads = [n_.enc(cc) for n_, _, cc in pairs], [n_.enc(cc, n_.grad) for n_, _, cc in pairs]
            ws, n3 = self._ebw_workspace(cs)
            if ws is None:
                ops.encoder_bwd(imgs, params, acts, douts, grads, H, W, self.compute, n=n3, xd=stage.image_flag(self.img_dtype),
                                device=self.dev)
                continue
            # per-image LDS-resident conv backward (encoder_bwd_fused.hip) as three calls
            np_, pk = len(pairs), int(self._prepacked)
            par_p, act_p, dout_p, grad_p, n_p = (ops.ptr_array(params), ops.ptr_array(acts), ops.ptr_array(douts), ops.ptr_array(grads),
                                                 ops.int_array(n3))
            # dependent chain: FC-tail input gradients (one launch) -> soft-argmax + conv backward
            call("tacorl_encoder_bwd_fused_head", np_, par_p, act_p, dout_p, n_p, H, W, pk, ptr(ws), ws.numel(), ops.stream())
            call("tacorl_encoder_bwd_fused_conv", np_, ops.ptr_array(imgs), par_p, act_p, grad_p, n_p, H, W, 0, pk, ptr(ws), ws.numel(),
                 ops.stream())
            # FC weight gradients last and in line: on a side branch they ran beside the conv-backward
            # kernels, whose 255 one-per-CU workgroups then no longer fit in one round (+0.13 ms/step)
            call("tacorl_encoder_bwd_fused_fc_wgrad", np_, act_p, dout_p, grad_p, n_p, H, W, 0, ptr(ws), ws.numel(),
                 ops.stream())

    def phase_c(self, optimize=True):
        """Optimiser steps (grads were all taken on the pre-step graph, as in the reference)."""
        hp, lap = self.hp, self.log_alpha_prime
        if optimize:
            a = self.actor
            items = [(lap.param, lap.grad, lap.m, lap.v, hp["critic_lr"], 0.0, lap.step, None, 0.0)] if self.with_lagrange else []
            items.append((a.param, a.grad, a.m, a.v, hp["actor_lr"], hp["clip"], a.step, None, 0.0))
            for q, t in ((self.q1, self.tq1), (self.q2, self.tq2)):
                items.append((q.param, q.grad, q.m, q.v, hp["critic_lr"], hp["clip"], q.step, t.param, hp["tau"]))
            ops.adam_step_batch(items)  # two launches for all blocks
            for c in self.enc_cams:  # (the fused encoder forward's packed conv weights, behind Adam: stage.PackedWeights)
                if self._fused_ok(c):
                    self.packs.pack([(n_, c) for n_ in self._late_pack_nets()])
        ops.mark("c:adam")

    def _allreduce(self, tensors):
        if D.collectives_on(self.world):
            for t in tensors:
                D.all_reduce_sum_(t)

    def metrics(self):
        """The logged scalars, read back (one D2H sync).  With several ranks they are first averaged over the ranks (one
        small collective on the steps that log): every slot is a per-rank batch mean or rank-independent, so the result is
        the full-batch value - what the reference's sync_dist=True logs give."""
        for fn in getattr(self, "pre_metrics", ()):  # device work only the logged scalars need (TACORL: the lazy action-decoder loss sum)
            fn()
        logs, div = D.reduce_logs_(self.logs, self.world)
        v = logs.cpu().tolist()
        # (the DR3 slots belong to an engine built with the term: without it nothing writes them and nothing logs them)
        return {k: x / div for k, x in zip(LOG_SLOTS, v) if k is not None and (self.dr3 is not None or k not in DR3_SLOTS)}
