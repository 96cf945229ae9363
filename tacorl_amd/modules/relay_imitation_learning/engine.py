"""Hand-scheduled relay-imitation-learning step (reference modules/relay_imitation_learning/relay_imitation_learning.py:
101-181) on HIP kernels: ONE perceptual encoder and ONE goal encoder shared by two behaviour-cloned policies.

    low  = -mean log pi_L(a_low                  | [e_low(obs)  | G(e_low(low_level_goal))])
    high = -mean log pi_H(G(e_high(hl_action))^  | [e_high(obs) | G(e_high(high_level_goal))])      (^ = no gradient)

Scheduled as the actor-critic engine schedules its step (tacorl_amd/engine.py), in a small engine of its own:

* per camera the images sit in four adjacent slots [obs | low_level_goal | high_level_goal | high_level_action] and are
  encoded once, by one network: 4*B images, activations saved for the first 3*B (the target rows have no backward);
* the goal encoder runs once over the three row sets ([low goal | high goal] with gradient, the target rows without);
* every parameter lives in ONE flat block: one gradient all-reduce, one Adam launch pair;
* no autograd, every buffer pre-allocated: the step is hipGraph-capturable (GraphMixin).
"""
import numpy as np
import torch

from ... import blocks, ops
from ... import encoder_stage as stage
from ... import image_ingest as ingest
from ... import dist as D
from ..._lib import ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH, BF16, F32, call, ptr

SLOTS = ("obs", "low_level_goal", "high_level_goal", "high_level_action")
N_GRAD_SLOTS = 3  # the leading slots whose images have a backward
LOG_SLOTS = ("low_level_loss", "high_level_loss")


class RILBlock:
    """[encoder(cam) for cam in cams] + goal-encoder MLP + high-level policy MLP + low-level policy MLP in one flat buffer,
    with the reference module's state-dict names as views."""

    def __init__(self, cams, genc_dims, pol_dims, pol_parts, device):
        self.cams = list(cams)
        self.genc_dims, self.pol_dims, self.pol_parts = list(genc_dims), dict(pol_dims), dict(pol_parts)
        off = 0
        self.enc_off = {}
        for c in self.cams:
            self.enc_off[c] = off
            off += blocks.encoder_size()
        self.genc_off = off
        off += blocks.mlp_size(self.genc_dims)
        self.pol_off = {}
        for k in ("high", "low"):
            self.pol_off[k] = off
            off += blocks.mlp_size(self.pol_dims[k])
        self.size = off
        z = lambda: torch.zeros(self.size, device=device)  # noqa: E731
        self.param, self.grad, self.m, self.v = z(), z(), z(), z()
        # bf16 copy of the goal encoder (the fused MLP forward's MFMA operand), refreshed every step
        self.param_bf16 = torch.zeros(self.size, device=device, dtype=torch.bfloat16)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.views, self.grad_views = self.views_of(self.param), self.views_of(self.grad)

    def views_of(self, flat):
        dst = {}
        for c in self.cams:
            for k, v in blocks.encoder_views(flat, self.enc_off[c]).items():
                dst[f"perceptual_encoder.networks.{c}.{k}"] = v
        gn = [(f"goal_encoder.mlp.{i}.weight", f"goal_encoder.mlp.{i}.bias") for i in (0, 2, 4)]
        dst.update(blocks.mlp_views(flat, self.genc_off, self.genc_dims, gn))
        for k in ("high", "low"):
            pre, dims = f"{k}_level_policy.policy.", self.pol_dims[k]
            names = [(f"{pre}fc_layers.{i}.weight", f"{pre}fc_layers.{i}.bias") for i in range(len(dims) - 2)]
            dst.update(blocks.mlp_views(flat, self.pol_off[k], dims[:-1], names))
            dst.update(blocks.head_views(flat, self.pol_off[k], dims, dims[-2], [(pre + n, r) for n, r in self.pol_parts[k]]))
        return dst

    def enc(self, cam, flat=None):
        return (self.param if flat is None else flat).data_ptr() + 4 * self.enc_off[cam]

    def genc(self, flat=None):
        return (self.param if flat is None else flat).data_ptr() + 4 * self.genc_off

    def genc_bf16(self):
        return self.param_bf16.data_ptr() + 2 * self.genc_off

    def pol(self, k, flat=None):
        return (self.param if flat is None else flat).data_ptr() + 4 * self.pol_off[k]


class RILEngine:
    def __init__(self, low_cams, high_cams, hw, B, device, *, lr=1e-4, goal_act="Tanh", goal_hidden=256, goal_out=32,
                 high=(4, 1024), low=(4, 1024), low_action_dim=7, low_discrete_gripper=True, compute=F32,
                 img_dtype=torch.float32, world_size=1):
        self.low_cams, self.high_cams = list(low_cams), list(high_cams)
        if sorted(self.low_cams) != sorted(self.high_cams) or len(set(self.low_cams)) != len(self.low_cams):
            raise ValueError(f"each modality list must be a permutation of the union: low {self.low_cams}, high {self.high_cams}")
        self.cams = list(self.low_cams)  # every camera the step encodes
        self.order = {"low": self.low_cams, "high": self.high_cams}
        self.dev, self.compute, self.img_dtype, self.world = device, compute, img_dtype, world_size
        self.hp = dict(lr=lr)
        self.Eo = self.G = 32 * len(self.cams)  # state embedding width = goal-encoder input width
        self.GO = goal_out
        self.E = self.Eo + self.GO
        self.genc_dims = [self.G, goal_hidden, goal_hidden, self.GO]
        self.genc_acts = [ACT_RELU, ACT_RELU, ACT_TANH if goal_act == "Tanh" else ACT_NONE]
        self.A_low, self.dg = low_action_dim, bool(low_discrete_gripper)
        # continuous action dims and head width [mean | log-std | gripper logits] of each policy
        self.Ac = {"high": self.GO, "low": low_action_dim - 1 if self.dg else low_action_dim}
        self.HD = {"high": 2 * self.GO, "low": 2 * self.Ac["low"] + (2 if self.dg else 0)}
        self.pol_dims = {k: [self.E] + [hid] * layers + [self.HD[k]] for k, (layers, hid) in (("high", high), ("low", low))}
        self.pol_acts = {k: [ACT_SILU] * (len(d) - 2) + [ACT_NONE] for k, d in self.pol_dims.items()}
        parts = {k: [("fc_mean", self.Ac[k]), ("fc_log_std", self.Ac[k])] for k in ("high", "low")}
        if self.dg:
            parts["low"].append(("gripper_action", 2))
        self.blk = RILBlock(self.cams, self.genc_dims, self.pol_dims, parts, device)
        self.packs = stage.PackedWeights(device)
        self.B, self.hw = None, dict(hw or {})
        if B:
            self.ensure_batch(B)

    # ------------------------------------------------------------------ buffers
    def ensure_batch(self, B, hw=None):
        hw = dict(hw) if hw is not None else self.hw
        if self.B != B or hw != self.hw:
            self.B, self.hw = B, hw
            self._alloc()

    def slot_rows(self):
        """{slot name: first image row in a camera's image buffer}; the first 3*B rows have a backward."""
        return {s: i * self.B for i, s in enumerate(SLOTS)}

    def enc_problems(self, c):
        """Encoder problems of camera c as (first image row, images, activations saved): one network, two row runs."""
        B = self.B
        return [(0, N_GRAD_SLOTS * B, True), (N_GRAD_SLOTS * B, B, False)]

    def _alloc(self):
        B, dev = self.B, self.dev
        ops.note_alloc()
        f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        ns = len(SLOTS)
        self.X3 = {c: torch.zeros(ns * B, *self.hw[c], 3, device=dev, dtype=self.img_dtype) for c in self.cams}
        self.enc_out = {c: f(ns * B, 32) for c in self.cams}
        self.enc_act = {c: f(ops.encoder_act_layout(N_GRAD_SLOTS * B, *self.hw[c])[1]) for c in self.cams}
        # (the per-layer encoder forward keeps its intermediate layers in the activation buffer: the target rows then need
        # one too; the fused launch writes nothing for them)
        self.enc_act_t = {c: None if self._fused_ok(c) else f(ops.encoder_act_layout(B, *self.hw[c])[1]) for c in self.cams}
        self.enc_dout = {c: f(N_GRAD_SLOTS * B, 32) for c in self.cams}
        gd, ga = self.genc_dims, self.genc_acts
        # goal encoder: problem 0 = rows [low goal | high goal] (backward), problem 1 = the high-level target rows
        self.gin, self.gin_t = f(2 * B, self.G), f(B, self.G)
        self.gact, self.gact_t = f(ops.mlp_act_layout(2 * B, gd, ga)[2]), f(ops.mlp_act_layout(B, gd, ga)[2])
        self.g_yoff, self.g_yoff_t = ops.mlp_act_layout(2 * B, gd, ga)[1][-1], ops.mlp_act_layout(B, gd, ga)[1][-1]
        # policy inputs / input gradients: rows [0, B) the low-level policy's, rows [B, 2B) the high-level policy's
        self.S, self.dS, self.dgin = f(2 * B, self.E), f(2 * B, self.E), f(2 * B, self.G)
        self.row0 = {"low": 0, "high": B}
        self.pact, self.p_yoff, self.d_head = {}, {}, {}
        for k in ("low", "high"):
            _, y, tot = ops.mlp_act_layout(B, self.pol_dims[k], self.pol_acts[k])
            self.pact[k], self.p_yoff[k], self.d_head[k] = f(tot), y[-1], f(B, self.HD[k])
        self.action = f(B, self.A_low)
        self.logs = f(4)

    # ------------------------------------------------------------------- inputs
    def load_images(self, cam, imgs, nchw=True):
        """imgs: the four slots' images in SLOTS order, each (B,3,H,W) fp32 [nchw], (B,H,W,3) fp32, or the dataset's
        uint8 (B,H,W,3) frames (ToTensor + Normalize(0.5, 0.5) applied by the pack, as ACEngine.load_images)."""
        ingest.pack_slots(self.X3[cam], range(len(SLOTS)), self.B, self.hw[cam], imgs, nchw, self.img_dtype)

    def load_action(self, action):
        self.action.copy_(action.reshape(self.B, self.A_low).float())

    # ------------------------------------------------------------------ encoder
    def _img_ptr(self, cam, first_row):
        H, W = self.hw[cam]
        return self.X3[cam].data_ptr() + first_row * H * W * 3 * self.X3[cam].element_size()

    def _fused_ok(self, c):
        return stage.fused_fwd_ok(self.hw[c], self.compute, self.img_dtype)

    def _fused_bwd_ok(self, c):
        return stage.fused_bwd_ok(self.hw[c], self.compute, self.img_dtype, [N_GRAD_SLOTS * self.B])

    def _fused_saves(self, c):
        return stage.fused_saves(self.hw[c], self.compute, self.img_dtype, [N_GRAD_SLOTS * self.B])

    def packs_stale(self):
        return self.packs.stale([self.blk], self.cams)

    def packs_written(self):
        self.packs.written([self.blk], self.cams)

    def _encode(self):
        """4*B images per camera through the one encoder: a fused launch per geometry group where it applies (activations
        saved for the first 3*B images only), the per-layer path otherwise - behind every fused launch.  ONE packed copy of
        the conv weights per camera (a single network): one pack launch per group."""
        def problems(c):
            return [(self._img_ptr(c, r0), self.blk, self.enc_out[c].data_ptr() + 4 * 32 * r0,
                     self.enc_act[c] if save else self.enc_act_t[c], n, save, c) for r0, n, save in self.enc_problems(c)]

        groups = stage.geometry_groups(self.cams, self.hw, self._fused_bwd_ok, lambda c: len(self.enc_problems(c)), stage.EF_MAXP)
        stage.encode(groups, problems, self.hw, self.compute, self.img_dtype, self.packs, self._fused_ok, self._fused_saves,
                     lambda c, pr: stage.launch_fused(pr, self.packs, self.hw[c]), pack_per_camera=False, per_layer_last=True)

    def _encoders_backward(self):
        """The encoder backward over the first 3*B images of every camera (one problem per camera)."""
        g = self.blk.grad
        for cs in stage.geometry_groups(self.cams, self.hw, self._fused_bwd_ok, lambda c: 1, stage.EBW_MAXP):
            fused = self._fused_bwd_ok(cs[0])
            ops.encoder_bwd([self._img_ptr(c, 0) for c in cs], [self.blk.enc(c) for c in cs], [self.enc_act[c] for c in cs],
                            [self.enc_dout[c] for c in cs], [self.blk.enc(c, g) for c in cs], *self.hw[cs[0]], self.compute,
                            fused=fused, n=[N_GRAD_SLOTS * self.B] * len(cs), xd=stage.image_flag(self.img_dtype), device=self.dev,
                            ws_tag="ril_enc_bwd_fused_" + "+".join(cs) if fused else "ril_enc_bwd")

    # ----------------------------------------------------------------- the step
    def mlp_paths(self):
        """Which MLP kernels the step's sites run: {site: "fused" / "per-layer"} (forward, backward)."""
        gd, B = self.genc_dims, self.B or 1
        out = {"goal_encoder": ("fused" if self.compute == BF16 and ops.L.lib().tacorl_mlp_fwd_fused_supported(
                                    2, len(gd) - 1, ops.int_array(gd), self.G) else "per-layer",
                                "fused" if ops.mlp_bwd_fused_ok(1, gd, self.E, self.G, self.compute) else "per-layer")}
        for k in ("low", "high"):
            out[k + "_level_policy"] = ("per-layer", "per-layer")
        return out

    def _head(self, k):
        return self.pact[k][self.p_yoff[k]: self.p_yoff[k] + self.B * self.HD[k]]

    def forward(self):
        """Encoders, goal encoder, both policies, both losses (+ dL/d head).  Everything validation needs."""
        B, E, G, GO, Eo, blk = self.B, self.E, self.G, self.GO, self.Eo, self.blk
        rows = self.slot_rows()
        self._encode()
        ops.mark("encode")
        bf = self.compute == BF16
        if bf:
            call("tacorl_to_bf16_batch", 1, ops.ptr_array([blk.genc()]), ops.ptr_array([blk.genc_bf16()]),
                 (ops.C.c_long * 1)(blocks.mlp_size(self.genc_dims)), ops.stream())
        # goal-encoder inputs: each role's embeddings concatenated in that role's list order
        with ops.copy_batch():
            for j, c in enumerate(self.low_cams):
                ops.copy_cols(self.enc_out[c], rows["low_level_goal"] * 32, 32, self.gin, 32 * j, G, B, 32)
            for j, c in enumerate(self.high_cams):
                ops.copy_cols(self.enc_out[c], rows["high_level_goal"] * 32, 32, self.gin, B * G + 32 * j, G, B, 32)
                ops.copy_cols(self.enc_out[c], rows["high_level_action"] * 32, 32, self.gin_t, 32 * j, G, B, 32)
        ops.mlp_fwd([self.gin, self.gin_t], G, [blk.genc()] * 2, [self.gact, self.gact_t], [2 * B, B], self.genc_dims,
                    self.genc_acts, self.compute, params_bf16=[blk.genc_bf16()] * 2 if bf else None)
        ops.mark("goal_encoder")
        # S = [enc(obs) in the policy's camera order | goal_enc(enc(goal))]
        with ops.copy_batch():
            for k in ("low", "high"):
                r0 = self.row0[k]
                for j, c in enumerate(self.order[k]):
                    ops.copy_cols(self.enc_out[c], rows["obs"] * 32, 32, self.S, r0 * E + 32 * j, E, B, 32)
                ops.copy_cols(self.gact, self.g_yoff + r0 * GO, GO, self.S, r0 * E + Eo, E, B, GO)
        # the two policies: one batched launch per layer when their shapes agree, else one MLP call each
        for ks in ([["low", "high"]] if self.pol_dims["low"] == self.pol_dims["high"] else [["low"], ["high"]]):
            ops.mlp_fwd([self.S[self.row0[k]: self.row0[k] + B] for k in ks], E, [blk.pol(k) for k in ks],
                        [self.pact[k] for k in ks], [B] * len(ks), self.pol_dims[ks[0]], self.pol_acts[ks[0]], self.compute)
        ops.mark("policies_fwd")
        gs = 1.0 / self.world
        call("tacorl_tanh_normal_nll", ptr(self._head("low")), self.HD["low"], ptr(self.action), self.A_low, B, self.Ac["low"],
             int(self.dg), gs, ptr(self.d_head["low"]), ops._at(self.logs, 0), ops.stream())
        call("tacorl_tanh_normal_nll", ptr(self._head("high")), self.HD["high"], ops._at(self.gact_t, self.g_yoff_t), GO, B,
             self.Ac["high"], 0, gs, ptr(self.d_head["high"]), ops._at(self.logs, 1), ops.stream())
        ops.mark("nll")

    def _mlp_backward(self, tag, *site):
        ops.mlp_backward(("ril_bwd_" + tag, "ril_bwdf_" + tag), *site, self.compute)

    def backward(self):
        B, E, G, Eo, blk = self.B, self.E, self.G, self.Eo, self.blk
        rows = self.slot_rows()
        g = blk.grad
        for ks in ([["low", "high"]] if self.pol_dims["low"] == self.pol_dims["high"] else [["low"], ["high"]]):
            sl = lambda t, k: t[self.row0[k]: self.row0[k] + B]  # noqa: E731
            self._mlp_backward("pol_" + ks[0], [sl(self.S, k) for k in ks], E, [blk.pol(k) for k in ks], [self.pact[k] for k in ks],
                               [self.d_head[k] for k in ks], self.HD[ks[0]], [blk.pol(k, g) for k in ks],
                               [sl(self.dS, k) for k in ks], E, [B] * len(ks), self.pol_dims[ks[0]], self.pol_acts[ks[0]])
        ops.mark("policies_bwd")
        # goal encoder: one problem over the 2*B rows that have a gradient (its weight gradients sum both policies' rows)
        self._mlp_backward("genc", [self.gin], G, [blk.genc()], [self.gact], [ops._at(self.dS, Eo)], E, [blk.genc(g)],
                           [self.dgin], G, [2 * B], self.genc_dims, self.genc_acts)
        ops.mark("goal_encoder_bwd")
        # embedding gradients per camera: rows [obs | low goal | high goal].  The obs rows are the SUM of the two policies'
        # contributions: the low-level policy's is copied, the high-level policy's accumulated by a second launch (the
        # copies of one batch must not read what another writes)
        with ops.copy_batch():
            for c in self.cams:
                jl, jh = self.low_cams.index(c), self.high_cams.index(c)
                ops.copy_cols(self.dS, 32 * jl, E, self.enc_dout[c], rows["obs"] * 32, 32, B, 32)
                ops.copy_cols(self.dgin, 32 * jl, G, self.enc_dout[c], rows["low_level_goal"] * 32, 32, B, 32)
                ops.copy_cols(self.dgin, B * G + 32 * jh, G, self.enc_dout[c], rows["high_level_goal"] * 32, 32, B, 32)
        with ops.copy_batch():
            for c in self.cams:
                ops.copy_cols(self.dS, B * E + 32 * self.high_cams.index(c), E, self.enc_dout[c], rows["obs"] * 32, 32, B, 32,
                              accumulate=True)
        self._encoders_backward()
        ops.mark("encoder_bwd")

    def optimizer_step(self):
        """One Adam over the whole block (no clipping), then the fused encoder's packed conv weights behind it."""
        b = self.blk
        ops.adam_step_batch([(b.param, b.grad, b.m, b.v, self.hp["lr"], 0.0, b.step, None, 0.0)])
        self.packs.pack([(b, c) for c in self.cams if self._fused_ok(c)])
        ops.mark("adam")

    def allreduce_grads(self):
        if D.collectives_on(self.world):
            D.all_reduce_sum_(self.blk.grad)

    def metrics(self):
        """{low_level_loss, high_level_loss, total_loss} read back (one D2H sync); averaged over the ranks first."""
        logs, div = D.reduce_logs_(self.logs, self.world)
        v = [x / div for x in logs.cpu().tolist()]
        out = dict(zip(LOG_SLOTS, v))
        out["total_loss"] = float(np.float32(v[0]) + np.float32(v[1]))
        return out
