"""RelayImitationLearning - drop-in for reference modules/relay_imitation_learning/relay_imitation_learning.py:13-225
(`experiment=relay_imitation_learning`, the hierarchical behaviour-cloning baseline).

Same constructor kwargs (`_recursive_: False`: sub-configs arrive as dicts), same `training_step / validation_step /
configure_optimizers` surface, same `state_dict()` keys and logged scalar names; the arithmetic runs in
tacorl_amd.modules.relay_imitation_learning.engine.RILEngine (HIP kernels).  Select it with
`module._target_=tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning.RelayImitationLearning`.

The reference optimises automatically (training_step returns the loss, the Trainer steps one Adam); here the Adam step is
part of training_step's kernels, so the module runs in manual-optimisation mode like the other three and returns the total
loss for logging only.  `env` is accepted and stored but never built (the reference calls make_env(env) and does not use it
in the step)."""
from typing import List

import torch

from ... import dist as _D
from ... import image_ingest as ingest
from ...lightning import LightningModuleBase
from ..common import GraphMixin, ModuleMixin, register_views, to_plain
from .engine import SLOTS, RILEngine


class RelayImitationLearning(GraphMixin, ModuleMixin, LightningModuleBase):
    def __init__(self, env={}, goal_encoder={}, perceptual_encoder={}, high_level_policy={}, low_level_policy={},
                 high_level_policy_modalities: List[str] = [], low_level_policy_modalities: List[str] = [],
                 lr: float = 1e-4, *args, device=None, compute_dtype="f32", image_dtype="f32", world_size=1, **kwargs):
        super().__init__()
        self._init_runtime(device, compute_dtype, image_dtype, world_size)
        self.automatic_optimization = False
        self.save_hyperparameters()
        self.env_cfg, self.env = env, None
        self.goal_encoder_cfg, self.perceptual_encoder_cfg = to_plain(goal_encoder), to_plain(perceptual_encoder)
        self.high_level_policy_cfg, self.low_level_policy_cfg = to_plain(high_level_policy), to_plain(low_level_policy)
        self.high_level_policy_modalities = list(high_level_policy_modalities)
        self.low_level_policy_modalities = list(low_level_policy_modalities)
        self.lr = lr
        self.build_networks()
        if _D.collectives_on(world_size):
            self.sync_from_rank0()

    # ------------------------------------------------------------------ construction
    def build_networks(self):
        from .. import cfgcheck
        from ...init import init_views_

        union = cfgcheck.check_ril_modalities(self.low_level_policy_modalities, self.high_level_policy_modalities)
        self.all_modalities = set(union)
        cfgcheck.check_representation(self.perceptual_encoder_cfg, "perceptual_encoder", union)
        g = self.goal_encoder_cfg or {}
        goal_act = cfgcheck.check_ril_goal_encoder(g, "goal_encoder", g.get("hidden_size", 256))
        goal_out = int(g.get("out_features") or 32)
        if g.get("in_features") not in (None, 32 * len(union)):
            raise ValueError(f"goal_encoder.in_features is 32 per camera of the union ({32 * len(union)}), not {g['in_features']}")
        hp, hdg, hA = cfgcheck.check_ril_policy(self.high_level_policy_cfg, "high_level_policy")
        lp, ldg, lA = cfgcheck.check_ril_policy(self.low_level_policy_cfg, "low_level_policy")
        if hdg:
            raise NotImplementedError("high_level_policy: discrete_gripper - its action is the latent goal, which has no gripper")
        if hA not in (None, goal_out):
            raise ValueError(f"high_level_policy.action_dim {hA} must equal goal_encoder.out_features {goal_out}")
        size = lambda p: (int(p.get("num_layers", 2)), int(p.get("hidden_dim", 256)))  # noqa: E731
        self.engine = RILEngine(
            self.low_level_policy_modalities, self.high_level_policy_modalities, None, None, self.dev, lr=self.lr,
            goal_act=goal_act, goal_hidden=int(g.get("hidden_size", 256)), goal_out=goal_out, high=size(hp), low=size(lp),
            low_action_dim=int(lA if lA is not None else 16), low_discrete_gripper=ldg, compute=self.compute,
            img_dtype=self.img_dtype, world_size=self.world_size)
        init_views_(self.engine.blk.views)
        self._pv = register_views(self, "", self.engine.blk.views)
        # rollout surface (evaluation/rollout_manager.py:434-557; evaluation/vec_policy.py RelayPolicy is built on it)
        from ..inference import attach_ril_rollout_surface

        attach_ril_rollout_surface(self, self.engine)

    def _blocks(self):
        return [self.engine.blk]

    def _stepped_blocks(self):
        return [self.engine.blk.param]

    def _derived_stale(self):
        return self.engine.packs_stale()

    def _after_replay_touch(self):
        self.engine.packs_written()

    def named_gradients(self):
        return dict(self.engine.blk.grad_views)

    # ---------------------------------------------------------------------- stepping
    def _stage(self, batch, nchw=True):
        """The four image roles of every camera of the union and the low-level action; fp32 NCHW tensors, or the
        dataset's uint8 HWC frames (normalised on the GPU, as CQL_Offline._stage).  Two more forms come from
        data/relay_replay.py: `batch["replay"]` (HbmRelayReplay.batch(fused=True): every image is read by frame id straight
        out of the resident dataset, row k of the (4, B) id table into slot k) and the gathered uint8 batch with
        `batch["aug"]`; both go through the pack CQL_Offline._stage_u8 uses, one launch of four jobs per camera."""
        e = self.engine
        rp, aug = batch.get("replay"), batch.get("aug")
        if rp is not None or aug is not None:
            slots = {s: k for k, s in enumerate(SLOTS)}
            if rp is not None:
                if rp.get("kind") != "relay":
                    raise ValueError("RelayImitationLearning takes the relay replay (HbmRelayReplay), not kind "
                                     f"{rp.get('kind')!r}")
                from ...data.replay import wait_ready

                wait_ready(batch)
                source = ingest.replay_source(rp, e.cams, slots, "relay replay batch")
                f = ingest.transition_form({c: rp["frames"][c] for c in e.cams}, aug=aug, replay=rp, rows=len(SLOTS))
            else:
                source = ingest.gathered_source(batch, {c: SLOTS for c in e.cams})
                f = ingest.transition_form({c: batch[SLOTS[0]][c] for c in e.cams}, aug=aug)
            e.ensure_batch(f.B, f.hw)
            ingest.pack_u8_roles(f, e.cams, e.X3, lambda c: slots, source, self.img_dtype)
            e.load_action(batch["low_level_action"].to(self.dev))
            return
        f = ingest.transition_form({c: batch[SLOTS[0]][c] for c in e.cams}, nchw)
        e.ensure_batch(f.B, f.hw)
        for c in e.cams:
            e.load_images(c, [batch[s][c].to(self.dev) for s in SLOTS], nchw=f.form == "f32_nchw")
        e.load_action(batch["low_level_action"].to(self.dev))

    def compute_loss(self, batch, stage: str = "train", optimize: bool = True):
        self._sync_lrs()
        self._stage(batch)
        e = self.engine

        def fwd_bwd():
            e.forward()
            if optimize:
                e.backward()

        def opt():
            if optimize:
                e.optimizer_step()

        self._run_segments(("ril", e.B, tuple(sorted(e.hw.items())), optimize), [fwd_bwd, opt],
                           [e.allreduce_grads if optimize else (lambda: None)])
        self._step_count += 1
        if self.log_every_n_steps > 1 and self._step_count % self.log_every_n_steps and self.__dict__.get("_last_total") is not None:
            return self.__dict__["_last_total"]
        m = e.metrics()
        for k in ("low_level_loss", "high_level_loss", "total_loss"):
            self.log(f"{stage}/{k}", m[k], on_step=True, on_epoch=True, sync_dist=True)
        self.__dict__["_last_total"] = m["total_loss"]
        return m["total_loss"]

    def training_step(self, batch, batch_idx=0):
        out = self.compute_loss(batch, stage="train", optimize=True)
        self._tick_optimizers()
        return out

    def validation_step(self, batch, batch_idx=0):
        return self.compute_loss(batch, stage="validation", optimize=False)

    def configure_optimizers(self):
        """reference :219-225: ONE Adam over every parameter - a BlockAdam over the flat block."""
        b = self.engine.blk
        self._optimizers = [self._make_adam("adam", [(b, self._pv, b.views_of(b.m), b.views_of(b.v))], self.lr)]
        return self._optimizers[0]

    def _sync_lrs(self):
        """A learning rate edited on the optimiser's param_groups reaches the kernels: it is a launch argument, so a change
        also drops the captured graphs."""
        opts = getattr(self, "_optimizers", None)
        if opts and opts[0].lr != self.engine.hp["lr"]:
            self.lr = self.engine.hp["lr"] = opts[0].lr
            self._graphs = {}

    def _set_world_size(self, ws):
        self.engine.world = ws
        super()._set_world_size(ws)
