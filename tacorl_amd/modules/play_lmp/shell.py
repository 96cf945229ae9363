"""The host shell of a PlayLMP step, stated once for image observations (play_lmp_for_rl.PlayLMP) and vector observations
(play_lmp_d4rl.PlayLMP): the Lightning surface, the one Adam over the three flat blocks, the gradient arena of the multi-GPU
all-reduce, the step's noise and the step itself around the class's own kernel sequence.  No arithmetic here.

A class says what differs:
  _parts()      [(key, block, state-dict prefix)] in arena / Adam-launch order; `_ref_name` where a view's state-dict name is
                not prefix + view name
  OPT_ORDER     the keys in optimiser-entry order (= the reference's parameter registration order; BlockAdam.state_dict()
                indexes parameters by position, so this order is checkpoint compatibility)
  LOG_NAMES     the names of the slots of self.logs (None: unused)
  GRAPH_KEY     the head of the step's graph key
  _open(batch, **form) -> B, T, rest of the shape key, batch form    (checks the batch, ensures the step's buffers)
  _stage(batch, form)  -> arguments of _fwd_bwd behind (B, T, gs)    (the batch into the fixed buffers)
  _fwd_bwd(B, T, gs, *args)                                          (the device side up to the gradients)"""
import torch

from ... import dist as D
from ... import ops


class PlayLMPShell:
    def _ref_name(self, name):
        return name

    def _blocks(self):
        return [blk for _, blk, _ in self._parts()]

    def set_kl_beta(self, kl_beta):
        """reference play_lmp_for_rl.py:303-305, play_lmp_d4rl.py:190-192."""
        if kl_beta != self.kl_beta:  # a launch argument of the KL kernel (a captured graph holds the old value) -> new captures
            self._graphs = {}
        self.kl_beta = kl_beta

    def last_plan_proposal(self):
        """The plan proposal of the most recent step as a distribution (what the reference's validation_step hands its
        callbacks a sample of: `sampled_plan_pp`): a TanhNormalDist over the proposal head where the step left it.
        Read-only: no launch is added to the step, and the head buffer is viewed, not copied - use it before the next step."""
        from ..inference import TanhNormalDist

        if getattr(self, "_shape", None) is None:
            raise RuntimeError("last_plan_proposal(): no step has run yet")
        B, A = self._shape[0], self.pr.A
        return TanhNormalDist(self.pact[self.p_yoff: self.p_yoff + B * 2 * A].view(B, 2 * A), A)

    def named_gradients(self):
        return {self._ref_name(p + k): v for _, blk, p in self._parts() for k, v in blk.grad_views.items()}

    def configure_optimizers(self):
        """reference play_lmp_for_rl.py:362-368, play_lmp_d4rl.py:235-241: ONE Adam over every parameter.  A BlockAdam spanning
        the three flat blocks."""
        blks = {k: blk for k, blk, _ in self._parts()}
        ent = [(blks[k], self._pv[k], blks[k].views_of(blks[k].m), blks[k].views_of(blks[k].v)) for k in self.OPT_ORDER]
        self._optimizers = [self._make_adam("adam", ent, self.lr)]
        return self._optimizers[0]

    def _grad_arena(self):
        """The three blocks' gradients as slices of one allocation (made on first use, i.e. only with several ranks)."""
        a = self.__dict__.get("_grad_arena_t")
        if a is None:
            ops.note_alloc()
            a = torch.zeros(sum(b.size for b in self._blocks()), device=self.dev)
            o = 0
            for b in self._blocks():
                b.rebind_grad(a[o: o + b.size])
                o += b.size
            self.__dict__["_grad_arena_t"] = a
        return a

    # --------------------------------------------------------------------------- the step's noise
    def carve_plan_noise(self, B, A):
        """The two draws (posterior sample eps_plan, random plan u_plan) in one flat buffer, with the entries of its
        device-noise segment table (the table itself is built at the first seeded draw: draw_plan_noise)."""
        n = (B * A + 3) // 4 * 4
        flat = self._noise_flat = torch.zeros(2 * n, device=self.dev)
        self.noise = dict(eps_plan=flat[:B * A].view(B, A), u_plan=flat[n: n + B * A].view(B, A))
        self._noise_entries = [("eps_plan", "normal", 0, (B, A)), ("u_plan", "uniform", n, (B, A))]
        self._noise_tables = {}

    def draw_plan_noise(self, noise, B, T):
        """The noise of a step, staged eagerly in front of its graph: the injected tape; or, with a device-noise seed, ONE
        tacorl_noise_fill launch for eps_plan, u_plan and - in train mode with dropout - the plan recognition's keep masks (the
        second destination base of that launch), after which the step counter advances; or torch's device generator."""
        pr = self.pr
        # plan-recognition dropout is live in train mode (reference transformer.yaml:9, nn.Module.training): its keep masks
        # are drawn (or injected: noise["dropout"]) here, with the step's other noise
        self._pr_train = bool(self.training and pr.dropout_p > 0)
        dn = self.__dict__.get("_device_noise")
        if noise is None and dn is not None:
            from ...noise import rank_sample0, table_for

            if self._pr_train:
                pr._ensure(B, T)
            tab = self._noise_tables.get(self._pr_train)
            if tab is None:
                tab = self._noise_tables[self._pr_train] = table_for(
                    self._noise_flat.numel(), self._noise_entries, B, pr.keep_flat.numel() if self._pr_train else 0,
                    pr.keep_entries if self._pr_train else ())
            dn.fill(tab, self._noise_flat, pr.keep_flat if self._pr_train else None, rank_sample0(B, self.world_size))
            dn.advance()
            return
        for k, buf in self.noise.items():
            if noise is not None:
                buf.copy_(noise[k].reshape(buf.shape))
            elif k.startswith("eps"):
                buf.normal_()
            else:
                buf.uniform_()
        if self._pr_train:
            pr.stage_dropout(B, T, noise.get("dropout") if noise is not None else None)

    # --------------------------------------------------------------------------- the step
    def _step(self, batch, noise=None, optimize=True, log_type="train", **form):
        """training_step + the single Adam (reference play_lmp_for_rl.py:200-257,307-317,362-368; play_lmp_d4rl.py:108-144,
        194-204)."""
        opts = getattr(self, "_optimizers", None)
        if opts and opts[0].lr != self.lr:  # lr edited on the optimiser (scheduler): a launch argument -> new captures
            self.lr, self._graphs = opts[0].lr, {}
        B, T, shape, f = self._open(batch, **form)
        gs = 1.0 / self.world_size
        # the step's draws, in the reference's order: dropout masks, rsample, one uniform_(-1, 1) random plan
        self.draw_plan_noise(noise, B, T)
        args = self._stage(batch, f)
        reduce_on = optimize and D.collectives_on(self.world_size)
        if reduce_on:
            self._grad_arena()  # (before anything is captured: the backward kernels write into the arena's slices)
        blocks = self._blocks()

        def opt():
            if optimize:
                ops.adam_step_batch([(blk.param, blk.grad, blk.m, blk.v, self.lr, 0.0, blk.step, None, 0.0) for blk in blocks])
            ops.mark("end")

        def reduce_grads():
            if reduce_on:
                D.all_reduce_sum_(self._grad_arena())  # ONE collective over the three blocks' gradients

        # (a graph replay runs no python: announce the optimiser's writes to torch's version counters - ops.touched)
        self._stepped_blocks = (lambda: [b.param for b in blocks]) if optimize else None
        self._run_segments((self.GRAPH_KEY, B, T, *shape, optimize, self._pr_train),
                           [lambda: self._fwd_bwd(B, T, gs, *args), opt], [reduce_grads])
        # metrics cross to the host (a device synchronisation) only on logging steps - Trainer(log_every_n_steps), as the
        # other modules do.  Deviation from the reference (which logs and returns the total on every step, :307-317): with
        # log_every_n_steps = k > 1 the train/* values - and their on_epoch means - come from every k-th step, and the steps
        # in between return the last total that was read (never None: the first step always reads).
        self._step_count += 1
        if (optimize and self.log_every_n_steps > 1 and self._step_count % self.log_every_n_steps
                and self.__dict__.get("_last_total") is not None):
            return self.__dict__["_last_total"]
        # (sync_dist=True in the reference, :162,183,292-339: the per-rank batch means are averaged over the ranks first)
        logs, div = D.reduce_logs_(self.logs, self.world_size)
        lg = [x / div for x in logs.cpu().tolist()]
        for k, v in zip(self.LOG_NAMES, lg):
            if k is not None:
                self.log(f"{log_type}/{k}", v, on_step=True, on_epoch=True, sync_dist=True)
        total = lg[1] + lg[2]
        self.log(f"{log_type}/total_loss", total, on_step=True, on_epoch=True, sync_dist=True)
        self.__dict__["_last_total"] = total
        return total

    def training_step(self, batch, batch_idx=0, noise=None):
        """reference :307-317 / :194-204 (returns the total loss; the optimiser step has already run - manual optimisation)."""
        out = self._step(batch, noise, True, "train")
        self._tick_optimizers()
        return out

    def validation_step(self, batch, batch_idx=0, noise=None):
        return self._step(batch, noise, False, "validation")
