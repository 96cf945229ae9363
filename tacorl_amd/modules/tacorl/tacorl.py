"""TACORL - drop-in for reference modules/tacorl/tacorl.py:21-300.

`training_step(batch)` = frozen LMP encoder over the B*T window frames -> plan-recognition
posterior -> sampled latent plan (the RL "action") -> (optional) action-decoder fine-tune ->
CQL update on (s, s', g) = (states[:,0], states[:,-1], goal), r = d = [disp == 1].
Select with `module._target_=tacorl_amd.modules.tacorl.tacorl.TACORL`.
"""
import torch

from ... import encoder_stage as stage
from ... import image_ingest as ingest
from ... import ops
from ..._lib import call, ptr
from ...encoder_stage import image_flag
from ..common import register_views
from ..cql.cql_offline_lightning import CQL_Offline
from .latent_plan import LatentPlanShell


class TACORL(LatentPlanShell, CQL_Offline):
    def __init__(self, *args, **kwargs):
        # The reference evaluates the action-decoder loss on every step even when the decoder is frozen,
        # although the value only reaches the logger (tacorl.py:206-233, optimize=False).  With
        # `action_loss_every_n_steps=k` that logging-only forward runs on every k-th step (match it to
        # Trainer(log_every_n_steps)); fine-tuning (`finetune_action_decoder=True`) always runs it.
        self.action_loss_every_n_steps = kwargs.pop("action_loss_every_n_steps", 1)
        super().__init__(*args, **kwargs)

    # ------------------------------------------------------------------ construction
    def build_networks(self):
        """reference tacorl.py:44-126."""
        from ..play_lmp.play_lmp_for_rl import PlayLMP, load_play_lmp

        lmp = self.__dict__.pop("_play_lmp", None)
        if lmp is None:
            lmp = load_play_lmp(self.play_lmp_dir, self.lmp_epoch_to_load, self.overwrite_lmp_cfg, device=self.dev,
                                compute_dtype=self.compute, image_dtype=self.img_dtype, unsafe_pickle=self.lmp_unsafe_pickle)
        assert isinstance(lmp, PlayLMP)
        from .. import cfgcheck

        cfgcheck.check_critic(self.critic_cfg, "critic")  # layers / hidden mirror the actor's (tacorl.py:72-73)
        cfgcheck.check_representation(self.critic_encoder_cfg, "critic_encoder", lmp.plan_proposal_obs_modalities)
        self.action_decoder_modalities = list(lmp.action_decoder_modalities)
        self.plan_recognition_modalities = list(lmp.plan_recognition_modalities)
        self.all_modalities = sorted(set(self.action_decoder_modalities + self.plan_recognition_modalities))
        cams, goal_cams = list(lmp.plan_proposal_obs_modalities), list(lmp.plan_proposal_goal_modalities)
        self.obs_modalities, self.goal_modalities = cams, goal_cams
        self.action_dim = lmp.pr.latent_plan_dim
        a = dict(policy_layers=lmp.policy_layers, q_layers=lmp.policy_layers, hidden=lmp.hidden,
                 discrete_gripper=False)  # critic q_network mirrors the actor's layers/hidden (tacorl.py:72-73)
        self._make_engine(cams, goal_cams, self.action_dim, a)
        e = self.engine
        # actor = deepcopy(LMP encoder) + deepcopy(LMP goal encoder) + LMP plan proposal (tacorl.py:63-70)
        e.actor.param.copy_(lmp.net.param)
        # critics: fresh encoders + fresh Q, goal encoders copied from the LMP (tacorl.py:93-120)
        from ...init import init_views_

        for q in (e.q1, e.q2):
            init_views_(q.views)
            n = q.head_off - q.genc_off
            q.param[q.genc_off: q.genc_off + n].copy_(lmp.net.param[lmp.net.genc_off: lmp.net.genc_off + n])
        self.sync_targets()
        self._register()
        # frozen LMP pieces (tacorl.py:51-53,124-126)
        self.lmp_net, self.pr, self.ad = lmp.net, lmp.pr, lmp.ad
        enc_views = {k[len("encoder."):]: v for k, v in lmp.net.views.items() if k.startswith("encoder.")}
        register_views(self, "perceptual_encoder.", enc_views, requires_grad=False)
        register_views(self, "plan_recognition.", lmp.pr.blk.views, requires_grad=False)
        if self.ad is not None:
            self._adopt_decoder()
        self._T = None
        # rollout surface (evaluation/rollout_manager.py:330-386): the frozen LMP encoder for the action decoder's state,
        # the decoder's one-step `act` with its carried hidden state
        from ..inference import attach_rollout_surface

        attach_rollout_surface(self, e.actor, cams, goal_cams, self.action_dim, False, lmp_net=self.lmp_net,
                               lmp_cams=self.action_decoder_modalities, ad=self.ad)

    # ---------------------------------------------------------------------- stepping
    def _ensure_seq(self, B, T, hw):
        if self._T == (B, T, tuple(sorted(hw.items()))):
            return
        ops.note_alloc()
        dev = self.dev
        self.frames = ingest.LazyImages({c: torch.zeros(B * T, *hw[c], 3, device=dev, dtype=self.img_dtype) for c in self.all_modalities})
        self.f_out = {c: torch.zeros(B * T, 32, device=dev) for c in self.all_modalities}
        self.f_act = {c: torch.zeros(ops.encoder_act_layout(B * T, *hw[c])[1], device=dev) for c in self.all_modalities}
        npr = len(self.plan_recognition_modalities)
        self.pr_in = torch.zeros(B * T, 32 * npr, device=dev)
        # the sampled plan IS the RL action and the displacement flag IS reward and done (get_rl_batch,
        # tacorl.py:142-179): alias the engine's transition buffers instead of copying into them every step
        e = self.engine
        assert e.action.shape == (B, self.action_dim) and e.action.dtype == torch.float32
        self.plan, self.reward = e.action, e.reward
        # the frozen LMP encoder over the B*T window frames rides in the engine's encoder launches
        self.engine.extra_enc = [dict(cam=c, img=self.frames.raw(c), net=self.lmp_net, out=self.f_out[c],
                                      act=self.f_act[c], n=B * T) for c in self.all_modalities]
        # entries [window | next] per camera for the batches whose forward-only images the encoder reads as fp32 (_fold_ok)
        self.src_tbl = {c: stage.SourceTable(dev, 2) for c in sorted(set(self.all_modalities) | set(self.engine.cams))}
        # ... and, for _step's batches, the whole front - those entries, the [obs; goal] pack, reward / done / action window -
        # as one table that the step's first graph node reads (_front_plan)
        self.front_tbl = stage.FrontTable(dev)
        self._folded = self._front = None
        self._T = (B, T, tuple(sorted(hw.items())))

    def _small_sources(self, batch, B):
        """(disp, its dtype code, the action window or None) where the transition kernel takes the batch's small tensors as they
        stand, else None."""
        disp, acts = batch["disp"], batch["actions"] if self.ad is not None else None
        dd = {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.uint8: 3, torch.bool: 3}.get(disp.dtype)
        if (dd is not None and disp.is_cuda and disp.is_contiguous() and disp.numel() == B
                and (acts is None or (acts.is_cuda and acts.is_contiguous() and acts.dtype == torch.float32
                                      and acts.shape == self.acts.shape))):
            return disp, dd, acts
        return None

    def _stage_small(self, batch, noise, B, T):
        e = self.engine
        disp, acts = batch["disp"], batch["actions"] if self.ad is not None else None
        small = self._small_sources(batch, B)
        if small is not None:
            dd = small[1]
            # reward = done = (disp == 1) and the action window, one launch
            call("tacorl_stage_transition", ptr(disp), dd, ptr(self.reward), ptr(e.done), B,
                 ptr(acts) if acts is not None else None, ptr(self.acts) if acts is not None else None,
                 acts.numel() if acts is not None else 0, ops.stream())
        else:
            if acts is not None:
                self.acts.copy_(acts)
            self.reward.copy_(disp == 1)
            e.done.copy_(self.reward)
        e.set_noise(noise)

    def _fold_ok(self, f, c, T, batch):
        """May camera c's forward-only images - the window frames of the frozen LMP encoder, the next observations of
        actor(next) and both targets - skip the pack?  The fused 84 x 84 forward then converts them itself, straight from the
        batch (tacorl_encoder_fwd_fused_src), and only [obs; goal], which conv1's weight gradient reads as packed bf16, are
        packed.  Needs: transformed fp32 CHW frames as they stand (no index table, no augmentation), bf16 compute on the fused
        kernel, 16-byte aligned tensors.  Everything else keeps the pack."""
        e, hw = self.engine, f.hw[c]
        if not (f.form == "f32_nchw" and f.aug is None and T >= 2 and e.use_fused and stage.fused_fwd_ok(hw, self.compute, self.img_dtype)):
            return False
        goal = batch["goal"][c] if c in e.cams else None
        if c in e.cams and not (c in e.slot and list(e.slot[c]) == ["obs", "goal", "next"] and goal.is_cuda and goal.is_contiguous()
                                and goal.dtype == torch.float32 and ingest.vector_ok(
                [ingest.PackJob(goal.data_ptr(), 3 * hw[0] * hw[1], 0, 1)], f.form, hw)):
            return False
        v, simg = f.frames[c], 3 * hw[0] * hw[1]
        return stage.SourceTable.ok(v.data_ptr(), simg, hw) and stage.SourceTable.ok(v.data_ptr() + 4 * (T - 1) * simg, T * simg, hw)

    def _front_plan(self, f, batch, B, T, cams_all, folded):
        """_step's batch on the fp32-source route, every camera folded: what the front table takes - (source entries
        [window | next] per camera of cams_all, pack jobs [obs; goal] per engine camera, the transition's arguments) - or None:
        a camera on the pack route, two geometries, small tensors the transition kernel does not take, too many cameras."""
        e, Job = self.engine, ingest.PackJob
        small = self._small_sources(batch, B)
        if not folded or folded != tuple(cams_all) or small is None or len({tuple(f.hw[c]) for c in cams_all}) != 1:
            return None
        disp, dd, acts = small
        sources, jobs = [], []
        for c in cams_all:
            src, simg = f.frames[c].data_ptr(), 3 * f.hw[c][0] * f.hw[c][1]
            sources += [(src, simg), (src + 4 * (T - 1) * simg, T * simg)]
            if c in e.cams:
                x3, slot = e.X3.raw(c).data_ptr(), B * simg * e.X3.raw(c).element_size()
                jobs += [Job(src, T * simg, x3, B), Job(batch["goal"][c].data_ptr(), simg, x3 + slot, B)]
        plan = (tuple(sources), tuple(jobs), disp.data_ptr(), dd, self.reward.data_ptr(), e.done.data_ptr(), B,
                acts.data_ptr() if acts is not None else None, self.acts.data_ptr() if acts is not None else None,
                acts.numel() if acts is not None else 0, tuple(f.hw[cams_all[0]]))
        return plan if self.front_tbl.accept(plan) else None

    def _stage_frames(self, batch, noise, nchw=True, fold=False, front=False):
        """Eager part of the step: pack the window frames (reference NCHW fp32 -> NHWC image dtype) into
        fixed buffers, copy the small tensors, draw / copy the noise.
        uint8 frames - the dataset's own format, (B, T, H, W, 3) with goal (B, H, W, 3) - are taken as they are
        and normalised on the way (ToTensor + Normalize(0.5, 0.5), bit-identical to the transformed fp32 frames).
        front (the caller runs _device_front next): where every camera takes the fp32-source route (fold), the [obs; goal]
        pack and the small tensors leave this eager part too - _device_front's first launch does them from the front table
        (_front_plan), and what stays here is the noise and, when an address moved, the table's fill."""
        from ...data.replay import wait_ready

        wait_ready(batch)  # a replay batch's small tables travel on the feeder's copy stream
        f = ingest.window_form(batch, nchw)
        B, T, hw, aug = f.B, f.T, f.hw, f.aug
        self.engine.extra_normal = {"eps_pr": (B, self.action_dim)}  # drawn with the engine's noise (one launch)
        self.engine.ensure_batch(B, {c: hw[c] for c in self.engine.cams})
        self.eps_pr = self.engine.extra_noise["eps_pr"]
        self._ensure_seq(B, T, hw)
        e = self.engine
        if self.ad is not None and (getattr(self, "acts", None) is None or self.acts.shape[:2] != (B, T)):
            ops.note_alloc()
            self.acts = torch.zeros(B, T, 7, device=self.dev)
        # the small launches of the eager part (reward / done / action window, the two noise generators) go beside the
        # HBM-bound image pack on a second stream instead of behind it
        if getattr(self, "_stage_stream", None) is None:
            self._stage_stream = torch.cuda.Stream(device=self.dev)
        main = torch.cuda.current_stream()
        u8, Job, ip = f.form in ingest.U8_FORMS, ingest.PackJob, None if f.ids is None else f.ids.data_ptr()
        cams_all = sorted(set(self.all_modalities) | set(e.cams))
        for c in cams_all:
            v = f.frames[c]
            assert v.is_cuda and v.is_contiguous() and v.dtype == (torch.uint8 if u8 else torch.float32)
        folded = tuple(c for c in cams_all if fold and self._fold_ok(f, c, T, batch))
        plan = self._front_plan(f, batch, B, T, cams_all, folded) if front else None
        if folded != self._folded or (plan is not None) != self._front:
            # (a captured step holds the route: a batch of another kind drops it)
            ops.note_alloc()
            self.front_tbl.invalidate()
            self._folded, self._front = folded, plan is not None
        side = self._stage_stream if getattr(self, "stage_side", True) else main
        if plan is not None:
            # the front table's route: the noise is all that is drawn here (torch's two generator launches), beside nothing -
            # hence on this stream, without the wait_stream pair (measured, profiles/step_front.md: on the side stream the
            # cross-queue join in front of the graph costs more than the pair of launches, 0.7686 against 0.7448 ms/step)
            side = main
            self.front_tbl.commit()  # (on main, behind the previous step's graph: it read the table)
            self._front_keep = (batch["goal"], batch["disp"], batch.get("actions"))  # (the step's first node reads them)
        if side is not main:
            side.wait_stream(main)  # the previous step's graph read these buffers
        with torch.cuda.stream(side):
            if plan is not None:
                e.set_noise(noise)
            else:
                self._stage_small(batch, noise, B, T)
        self.frames.drop()  # (what the previous batch left for a reader is superseded)
        e.X3.drop()
        tbl_i = {c: i for i, c in enumerate(cams_all)}
        entry = (lambda c, k: self.front_tbl.entry(tbl_i[c], k)) if plan is not None else (lambda c, k: self.src_tbl[c].entry(k))
        e.fp_src = {c: {"next": entry(c, 1)} for c in folded if c in e.cams}
        for x in e.extra_enc:
            x["src"] = entry(x["cam"], 0) if x["cam"] in folded else None
        for c in cams_all:
            v = f.frames[c]
            src, simg = v.data_ptr(), 3 * f.src_hw[c][0] * f.src_hw[c][1]  # (simg: elements of a source frame)
            if c in folded:
                # entries [window | next = window frame T - 1]; of the images only s = states[:, 0] and the goal are packed
                if plan is None:
                    self.src_tbl[c].fill([(src, simg), (src + 4 * (T - 1) * simg, T * simg)], hw[c])
                form, shw = f.form, f.src_hw[c]
                later = lambda jobs, c=c, keep=v, form=form, shw=shw: ingest.pack(jobs, form, self.img_dtype, shw, hw[c])  # noqa: E731 (keep: the batch tensor stays alive for a reader)
                if c in self.all_modalities:
                    self.frames.defer(c, lambda c=c, later=later, src=src, simg=simg: later([Job(src, simg, self.frames.raw(c).data_ptr(), B * T)]))
                if c in e.cams:
                    x3, slot = e.X3.raw(c).data_ptr(), B * 3 * hw[c][0] * hw[c][1] * e.X3.raw(c).element_size()
                    if plan is None:  # (else: the front table's pack jobs, _device_front's first launch)
                        ingest.pack([Job(src, T * simg, x3, B), Job(batch["goal"][c].data_ptr(), simg, x3 + slot, B)], form, self.img_dtype, shw, hw[c])
                    e.X3.defer(c, lambda later=later, src=src, simg=simg, x3=x3, slot=slot: later([Job(src + 4 * (T - 1) * simg, T * simg, x3 + 2 * slot, B)]))
                continue
            jobs, roles = [], []
            if c in self.all_modalities:  # a camera's jobs: the window into self.frames ...
                jobs, roles = [Job(src, simg, self.frames.raw(c).data_ptr(), B * T, ip, 1)], ["window"]
            if c in e.cams:  # ... and s = states[:,0], the goal, s' = states[:,-1] (get_rl_batch, tacorl.py:142-179) into X3's slots
                x3, slot = e.X3.raw(c).data_ptr(), B * 3 * hw[c][0] * hw[c][1] * e.X3.raw(c).element_size()
                if ip is not None:  # by index (ids[i * stride]): obs = ids[b T], goal = the table's tail, next = ids[b T + T - 1]
                    jobs += [Job(src, simg, x3, B, ip, T), Job(src, simg, x3 + slot, B, ip + 8 * B * T, 1),
                             Job(src, simg, x3 + 2 * slot, B, ip + 8 * (T - 1), T)]
                else:  # strided views of the window
                    g = batch["goal"][c]
                    assert g.is_cuda and g.is_contiguous() and g.dtype == v.dtype
                    jobs += [Job(src, T * simg, x3, B), Job(g.data_ptr(), simg, x3 + slot, B),
                             Job(src + v.element_size() * (T - 1) * simg, T * simg, x3 + 2 * slot, B)]
                roles += ["obs", "goal", "next"]
            if aug is not None:  # train-time augmentations on the way in: the draws arrive as device tables
                jobs = [j._replace(**ingest.window_tables(aug, c, r, T)) for j, r in zip(jobs, roles)]
            if len(jobs) == 4 and T >= 2 and ingest.vector_ok(jobs, f.form, hw[c]):
                ingest.pack_window(jobs, T, self.img_dtype, hw[c])  # one read of the window for its frames, obs and next
            else:
                ingest.pack(jobs, f.form, self.img_dtype, f.src_hw[c], hw[c], aug["pad"][c] if aug is not None else None)
        if side is not main:
            main.wait_stream(side)
        return B, T, hw

    def _ad_due(self):
        k = self.action_loss_every_n_steps
        return self.ad is not None and (self.finetune_action_decoder or k <= 1 or (self._step_count + 1) % k == 0)

    def _device_front(self, B, T, hw, optimize, with_ad=True):
        """Graph-capturable: all encoders (frozen LMP + actor/critics/targets) -> plan recognition -> plan ->
        AD loss -> first phase of the CQL update (up to the alpha gradient)."""
        e = self.engine
        ops.mark("front:start")
        if self._front:  # [obs; goal] pack, reward / done, action window: one node that follows the batch through the table
            self.front_tbl.launch()
        if getattr(self, "_pr_stream", None) is None:
            self._pr_stream, self._side_stream = torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)
        main = torch.cuda.current_stream()
        mods = self.plan_recognition_modalities
        # one camera: the frame embeddings are the transformer's input as they stand
        emb, ld = (self.f_out[mods[0]], 32) if len(mods) == 1 else (self.pr_in, self.pr_in.shape[1])
        # fine-tuning: the decoder's weights-only preparation (bf16 mirrors, transposed copies for BPTT and the heads' input
        # gradient: ~45 us at the head of the decoder's chain, which is the step's critical path in C3) beside the encoders
        ad_prep, ad_prepared = None, False
        if (with_ad and optimize and self.finetune_action_decoder and getattr(self, "ad_early_prepare", True)
                and self.ad._bwd_fast(B, self.compute)):
            self._side_stream.wait_stream(main)
            with torch.cuda.stream(self._side_stream):
                self.ad.refresh_mirrors(B, T - 1)
                ad_prepared = self.ad.prepare_backward(B, T - 1, self.compute)
                ad_prep = torch.cuda.Event()
                ad_prep.record(self._side_stream)
        # The frozen LMP window's encoder problems as a launch of their own FIRST, the plan recognition -> action decoder
        # branch forked right behind it, the update's own encoder problems after that on 160 workgroups (engine.encode_split):
        # where that branch is the step's longer chain it starts ~80 us earlier.  Measured (round 5): C4's share (window 32: 33
        # recurrent launches of 64 rows; `ad:end` 1 017 us against `c:adam` 864) 1.274 - 1.293 -> 1.222 - 1.238 ms/step in six
        # of seven runs (one read 1.337: whose workgroups get the freed CUs first is a race); the headline step (window 16,
        # balanced chains) +12 us; the same step with the decoder fine-tuned (C3: loss, BPTT, weight gradients and Adam make
        # that branch the critical one) 1.518 -> 1.497.  Hence: windows of 24 steps and more, or a fine-tuned decoder.
        split = with_ad and (T >= 24 or (optimize and self.finetune_action_decoder))
        forked = []

        def fork_branches():
            forked.append(self._fork_pr_ad(B, T, main, mods, emb, ld, with_ad, optimize, ad_prep, ad_prepared))

        if not (split and e.encode_split(fork_branches)):
            e._encode_all()
        ops.mark("front:encoded")
        if not forked:
            fork_branches()
        ready, ad_on_side = forked[0]
        e.action_ready = ready
        e.phase_a(encoded=True, optimize=optimize)
        if ad_prep is not None:
            main.wait_stream(self._side_stream)  # (every forked stream joins the capture's origin)
        segmented = self._segmented() or not self._use_graph
        if with_ad and not ad_on_side:
            if segmented:
                main.wait_stream(self._pr_stream)
            else:
                # one graph for the whole step: the fine-tuning chain (loss, BPTT, weight gradients, Adam - 1.4 ms, touching
                # nothing but the decoder's own buffers) stays a branch beside the CQL update and joins at the end of the step -
                # or, with the collectives captured inside that graph (several ranks), in front of the SECOND all-reduce, whose
                # arena holds the decoder's gradients (round 6: it used to join here, in front of the first one - the whole
                # decoder chain then stood between phase_a and phase_b: 1.078 against 0.864 ms at C3's B = 32 share)
                self._ad_join = self._pr_stream
        if segmented:
            # every segment must be self-contained (its graph is replayed on its own)
            main.wait_stream(self._pr_stream)
            e.action_ready = None
            self._join_ad()

    def _fork_pr_ad(self, B, T, main, mods, emb, ld, with_ad, optimize, ad_prep, ad_prepared):
        """The plan recognition -> plan -> action-decoder branches of the step, forked from `main` where it stands.  Returns
        (the event "plan / RL action written", whether the decoder pass runs on the second side stream)."""
        e = self.engine
        # Plan recognition -> plan -> (action-decoder loss) only need the frame embeddings; the first phase of
        # the CQL update does not need the plan.  They run as parallel branches of the step's graph:
        #   side stream 1: PR transformer -> sampled plan (= the RL action, in place) -> event action_ready
        #   side stream 2 (forked after the plan): frozen action-decoder forward + loss (logging only)
        #   main stream  : policy / sampling / alpha (phase_a); phase_b waits for action_ready
        self._ad_join = None
        ad_on_side = with_ad and not (optimize and self.finetune_action_decoder)
        self._pr_stream.wait_stream(main)
        with torch.cuda.stream(self._pr_stream):
            ops.mark("pr:start")
            if len(mods) > 1:
                for j, c in enumerate(mods):
                    ops.copy_cols(self.f_out[c], 0, 32, self.pr_in, 32 * j, self.pr_in.shape[1], B * T, 32)
            # the frozen decoder pass on the ring route reads bf16 rows [plan | frame embedding | 0]: the launch that samples
            # the plan writes them (one launch less at the head of the decoder branch, which ends the step)
            ad_rows = None
            if (ad_on_side and not self.finetune_action_decoder and getattr(self, "pr_writes_ad_rows", True)
                    and getattr(self.pr, "writes_ad_rows", False)):
                xb_seq, ad_emb = self.ad.ring_rows(B, T - 1, self.compute), self.ad.module_emb(self, B, T, gather=False)
                if xb_seq is not None and ad_emb is not None:
                    ad_rows = (xb_seq, T - 1, self.ad.P, self.ad.E, ad_emb[0], ad_emb[1])
            # the LMP networks are frozen in TACORL (tacorl.py:52-66): their weight-only preparation is cached
            self.pr.forward(emb, ld, B, T, self.compute, inference=True, sample=(self.eps_pr, self.plan), frozen=True,
                            **({} if ad_rows is None else {"ad_rows": ad_rows}))
            rows_current = bool(getattr(self.pr, "rows_written", False))
            ops.mark("pr:plan")
            ready = torch.cuda.Event()
            ready.record(self._pr_stream)
            if with_ad and not ad_on_side:
                # fine-tuning: loss + BPTT (+ Adam on one GPU) stay in line on this branch.  With more than one GPU the
                # decoder's gradient block is part of the engine's arena: the step's second all-reduce covers it and
                # the Adam step follows in the last segment (reference tacorl.py:206-233 has no dependency
                # between this update and the CQL update)
                if ad_prep is not None:
                    self._pr_stream.wait_event(ad_prep)
                self.ad.loss_step(self, self.acts, self.plan, B, T, True, defer_update=self._defer_ad_update(),
                                  mirrors_current=ad_prep is not None, prepared=ad_prepared)
        if ad_on_side:
            # compute_action_decoder_update (tacorl.py:206-233), frozen decoder: 30 small dependent GEMMs that each
            # fill a fraction of the chip -> their own branch, joined at the end of the step
            self._side_stream.wait_event(ready)
            with torch.cuda.stream(self._side_stream):
                ops.mark("ad:start")
                self.ad.loss_step(self, self.acts, self.plan, B, T, False, frozen=not self.finetune_action_decoder,
                                  rows_current=rows_current)
                ops.mark("ad:end")
            self._ad_join = self._side_stream
        return ready, ad_on_side

    def get_pr_latent_plan(self, batch, noise=None, nchw=True):
        """reference tacorl.py:235-252 (no_grad / eval): returns the sampled latent plan (device tensor)."""
        B, T, hw = self._stage_frames(batch, noise, nchw)
        xd = image_flag(self.img_dtype)
        for c in self.all_modalities:
            H, W = hw[c]
            call("tacorl_encoder_fwd", 1, ops.ptr_array([self.frames[c]]), ops.ptr_array([self.lmp_net.enc(c)]),
                 ops.ptr_array([self.f_out[c]]), ops.ptr_array([self.f_act[c]]), ops.int_array([B * T]), H, W, xd,
                 self.compute, ops.stream())
        for j, c in enumerate(self.plan_recognition_modalities):
            ops.copy_cols(self.f_out[c], 0, 32, self.pr_in, 32 * j, self.pr_in.shape[1], B * T, 32)
        head = self.pr.forward(self.pr_in, self.pr_in.shape[1], B, T, self.compute, inference=True)
        call("tacorl_pr_sample", ptr(head), ptr(self.eps_pr), ptr(self.plan), None, None, B, self.action_dim,
             float(self.pr.min_std), ops.stream())
        return self.plan

    def _step(self, batch, noise, optimize, log_type, nchw=True):
        # (the front table serves the step that is ONE graph, or eager.  The step split into graph segments with eager
        # collectives between them keeps the eager front: with the table its logging-only decoder pass, a side graph, no
        # longer ran beside the segments - 0.85 -> 1.11 ms at B = 256, profiles/step_front.md section 6)
        B, T, hw = self._stage_frames(batch, noise, nchw, fold=getattr(self, "fp32_ingest", True), front=not self._segmented())
        with_ad = self._ad_due()
        key = ("tacorl", B, T, tuple(sorted(hw.items())), self.current_epoch < self.bc_epochs, optimize, with_ad)
        e, bc = self.engine, self.current_epoch < self.bc_epochs
        ad_update = with_ad and optimize and self.finetune_action_decoder and self._defer_ad_update()

        def tail():
            e.phase_c(optimize)
            self._join_ad()
            if ad_update:
                self.ad.update(self)  # its gradients came through the second all-reduce with the arena
            ops.mark("step:end")

        # split (multi-GPU) graphs: the frozen, logging-only action-decoder pass leaves the first segment
        # and runs as a side graph beside the all-reduces and the other segments
        segmented = self._segmented()
        ad_ft = optimize and self.finetune_action_decoder
        ad_side = with_ad and segmented and self._use_graph
        # (round 6: the FINE-TUNED decoder's loss + backward as the side graph too - joined in front of all-reduce #2, whose arena
        # holds its gradients; inside the first segment its chain, the step's longest, stood in front of phase_b)
        side = None
        if ad_side and ad_ft:
            side = (0, lambda: self.ad.loss_step(self, self.acts, self.plan, B, T, True, defer_update=True), 1)
        elif ad_side:
            side = (0, lambda: self.ad.loss_step(self, self.acts, self.plan, B, T, False, frozen=not self.finetune_action_decoder))
        def allreduce_grads():
            if ad_update:  # a fine-tuned decoder's branch: its gradient block is part of the arena (the frozen, logging-only
                self._join_ad()  # pass keeps running beside the all-reduce and the optimiser and joins at the end of the step)
            e.allreduce_grads()

        self._run_segments(key, [lambda: self._device_front(B, T, hw, optimize, with_ad and not ad_side),
                                 lambda: e.phase_b(bc, optimize), tail],
                           [e.allreduce_alpha, allreduce_grads], side=side)
        self._publish_logs(log_type, extra=("action_loss",) if with_ad else ())
