"""Latent-plan policies rolled out for many environments in one step - the inner loop of the reference's rollout managers
(evaluation/rollout_manager.py:232-283 LatentPlanRollout, :361-407 TACORL; rollout_manager_d4rl.py:137-157, :206-241) for R
environments whose episodes end and whose plans renew at different steps:

    policy = LatentPlanPolicy(module, n_envs=R, plan_duration=16)
    policy.reset()                                   # every row re-plans on its next step
    actions = policy.step(observation, goal)         # (R, A) fp32 on the device
    infos = rollout_episodes(policy, envs)           # one episode per environment, all at once

A row re-plans on its first step after `reset` and every `plan_duration` steps after that; re-planning restarts that row's
decoder state (the reference's `clear_hidden_state()`).  The clock is plain host integers, so nothing is read back from
the device to decide anything.  The plan comes from `actor.get_actions(deterministic=True)` where the module has an actor
(TACORL; refined by CEMOptimizer with use_cem), from `plan_proposal.get_dist(...).sample()` otherwise (PlayLMP); only the
rows that re-plan go through it.  The decoder step is ActionDecoderLogistic.step_rows: per-row hidden state, one
tacorl_rows_linear2_fwd per layer up to 16 rows, and above that - where the training GEMMs are the faster ones
(profiles/vec_rollout.md) - the kernels `act` is made of, the restarted rows zeroed first.  Nothing is captured in a hipGraph.

`latent_plan_policy_restatement` states the same schedule in plain torch ops over callables, for any device and dtype:
the yardstick of tests/test_vec_policy_cpu.py (as modules/cem.py's cem_restatement is for the CEM kernel).

`RelayPolicy` / `relay_policy_restatement` below are the same for RelayImitationLearning (rollout_manager.py:434-557): the same
clock, a latent sub-goal from the high-level policy in place of the plan, the low-level policy in place of the decoder, no
recurrent state.  `rollout_episodes` drives either policy, one episode per environment; `rollout_episodes_refill` runs a queue
of episodes over the environments and refills a slot the step after its episode ends (the long-horizon evaluation).

`RLPolicy` / `rl_policy_restatement` are the flat baseline (rollout_manager.py:81-180 RLRollout): one deterministic
`actor.get_actions` per row per step, refined by CEMOptimizer under use_cem; no clock and no state.

Every `step` takes `embeddings=` in place of images: what evaluation/frame_ingest.py FrameIngest makes of the environments' raw
uint8 frames - per network the observation embeddings {camera: (R,32)} of this step and the per-row cache of goal embeddings.
With embeddings=None a step runs exactly as it did without the argument.
"""
import numpy as np
import torch


class PlanClock:
    """The per-row schedule in host integers: steps since the row's plan was made (None: re-plan on the next step)."""

    def __init__(self, n_rows, plan_duration):
        if n_rows < 1 or plan_duration < 1:
            raise ValueError(f"n_rows {n_rows}, plan_duration {plan_duration}")
        self.n, self.duration = int(n_rows), int(plan_duration)
        self.age = [None] * self.n

    def reset(self, rows=None):
        for r in _row_list(rows, self.n):
            self.age[r] = None

    def due(self):
        """Rows that re-plan (and restart their decoder state) on this step."""
        return [r for r in range(self.n) if self.age[r] is None or self.age[r] >= self.duration]

    def tick(self, replanned):
        for r in range(self.n):
            self.age[r] = 1 if r in replanned else self.age[r] + 1


def _row_list(rows, n):
    if rows is None:
        return list(range(n))
    if isinstance(rows, torch.Tensor):
        rows = rows.cpu().tolist()
    rows = list(rows)
    if len(rows) == n and all(isinstance(v, (bool, np.bool_)) for v in rows):
        return [r for r in range(n) if rows[r]]
    out = [int(r) for r in rows]
    if any(r < 0 or r >= n for r in out):
        raise IndexError(f"rows {out} of {n}")
    return out


def _take(x, idx):
    """Rows idx (a device index tensor) of a tensor or of a {camera: tensor} dict."""
    if isinstance(x, dict):
        return {k: _take(v, idx) for k, v in x.items()}
    return x.index_select(0, idx)


def _cat_rows(d, cams, idx=None):
    """The {camera: (R,32)} embeddings of `cams` side by side, as state_from_observation concatenates them; rows idx of it."""
    x = d[cams[0]] if len(cams) == 1 else torch.cat([d[c] for c in cams], dim=-1)
    return x if idx is None else x.index_select(0, idx)


def _obs_goal_rows(owner, net, emb, name, cams, goal_cams, idx=None):
    """[enc(obs) | goal_encoder(enc(goal))] of network `name` out of a step's embeddings: the second half of
    ActorSurface / CriticSurface.emb_representation (modules/inference.py), the same launch on the same rows."""
    from .. import ops

    e_obs = _cat_rows(emb.obs[name], cams, idx)
    if not goal_cams:
        return e_obs
    e_goal = _cat_rows(emb.goal[name], goal_cams, idx).contiguous()
    n = e_obs.shape[0]
    lay = ops.mlp_act_layout(n, net.genc_dims, net.genc_acts)
    gact = torch.zeros(lay[2], device=owner.dev)
    ops.mlp_fwd([e_goal], e_goal.shape[1], [net.genc()], [gact], [n], net.genc_dims, net.genc_acts, owner.compute)
    yo = lay[1][-1]
    return torch.cat([e_obs, gact[yo: yo + n * net.G].view(n, net.G)], dim=-1)


def _critic_rows(module, emb, idx=None):
    """What CEMOptimizer maximises over, out of a step's embeddings: q1's own [enc(obs) | goal_encoder(enc(goal))]."""
    cs = module.q1.__dict__["critic_surface"]
    return _obs_goal_rows(module, cs.net, emb, "q1", cs.cams, cs.goal_cams, idx)


class LatentPlanPolicy:
    def __init__(self, module, n_envs, plan_duration=16, use_cem=False, cem_kwargs=None):
        self.module, self.R = module, int(n_envs)
        self.ad = getattr(module, "ad", None)
        if self.ad is None:
            raise ValueError("the module has no action decoder")
        self.dev = module.dev
        self.clock = PlanClock(n_envs, plan_duration)
        self.plan_duration = int(plan_duration)
        self.image = bool(getattr(module, "action_decoder_modalities", None))
        actor = getattr(module, "actor", None)
        self.actor = actor if getattr(actor, "get_actions", None) is not None else None
        if self.actor is None and getattr(getattr(module, "plan_proposal", None), "get_dist", None) is None:
            raise ValueError("the module has neither actor.get_actions nor plan_proposal.get_dist")
        self.cem = None
        if use_cem:
            if self.actor is None:
                raise ValueError("use_cem needs a module with an actor and critics (TACORL)")
            from ..modules.cem import CEMOptimizer

            self.cem = CEMOptimizer(q1=module.q1, q2=module.q2, action_dim=self.actor.action_dim, discrete_gripper=False,
                                    **(cem_kwargs or {}))
        self.state = self.ad.new_rows_state(self.R)
        self.plan = torch.zeros(self.R, self.ad.P, device=self.dev)

    def reset(self, rows=None):
        """All rows, or an index list / bool mask: those rows re-plan (and start from h_0 = 0) on their next step."""
        self.clock.reset(rows)

    @property
    def hidden(self):
        return self.state.hidden

    # ------------------------------------------------------------------ plan source
    def _source_embedded(self, emb, idx, eps, cem_eps=None):
        """_source on a step's embeddings (FrameIngest) in place of images."""
        m = self.module
        if self.actor is not None:
            surf = m.__dict__["_actor_surface"]
            o = _obs_goal_rows(m, surf.net, emb, "actor", surf.cams, surf.goal_cams, idx)
            plan, _ = self.actor.get_actions(o, deterministic=True, reparameterize=False)
            if self.cem is not None:
                plan = self.cem.get_action(obs=_critic_rows(m, emb, idx), initial_mean=plan,
                                           noise=None if cem_eps is None else {"eps": cem_eps})
            return plan
        state = _cat_rows(emb.obs["lmp"], m.plan_proposal_obs_modalities, idx)
        pp_goal = m.goal_encoder(_cat_rows(emb.goal["lmp"], m.plan_proposal_goal_modalities, idx))
        return m.plan_proposal.get_dist(state_emb=state, goal_emb=pp_goal).sample(noise=eps)

    def _source(self, observation, goal, idx, eps, cem_eps=None):
        """The plan of rows idx: (len(idx), P)."""
        m = self.module
        obs, g = _take(observation, idx), _take(goal, idx)
        if self.actor is not None:
            o = {"observation": obs, "goal": g} if self.image else torch.cat([obs, g], dim=-1)
            plan, _ = self.actor.get_actions(o, deterministic=True, reparameterize=False)
            if self.cem is not None:
                plan = self.cem.get_action(obs=o, initial_mean=plan, noise=None if cem_eps is None else {"eps": cem_eps})
            return plan
        if self.image:
            pe = m.perceptual_encoder
            state = pe.get_state_from_observation(observation=obs, modalities=m.plan_proposal_obs_modalities)
            pp_goal = m.goal_encoder(pe.get_state_from_observation(observation=g, modalities=m.plan_proposal_goal_modalities))
        else:
            state, pp_goal = obs, g
        return m.plan_proposal.get_dist(state_emb=state, goal_emb=pp_goal).sample(noise=eps)

    def step(self, observation, goal, noise=None, plans=None, embeddings=None):
        """observation / goal: {camera: (R,3,H,W)} fp32 dicts (image modules) or (R,S) / (R,G) tensors (D4RL).  noise: any
        subset of {"plan_eps": (R,P), "rand_a": (R,Da,K), "rand_b": (R,Da), "cem_eps": (R,iters,N,P)}; the rest is drawn on the
        device.  plans: (R,P) with NaN rows meaning "not given" - overrides the plan source for the rows that re-plan (an
        external planner).  embeddings: a FrameIngest step's result, in place of observation / goal (image modules; both may then be None).
        Returns the (R, A) actions: a view that stays valid until the next step."""
        R, dev, noise = self.R, self.dev, noise or {}
        if embeddings is not None:
            if not self.image:
                raise ValueError("embeddings= stands in for images: this module takes vector observations")
        else:
            to = lambda x: ({k: to(v) for k, v in x.items()} if isinstance(x, dict) else torch.as_tensor(x).to(dev, torch.float32))  # noqa: E731
            observation, goal = to(observation), to(goal)
        due = self.clock.due()
        if due:
            need = due
            if plans is not None and not plans.is_cuda:  # a host tensor: which rows it gives is known without a device read
                given = (~torch.isnan(plans.reshape(R, -1)).any(dim=1)).tolist()
                need = [r for r in due if not given[r]]
            idx = torch.tensor(due, dtype=torch.long, device=dev)
            new = None
            if need:
                nidx = idx if need == due else torch.tensor(need, dtype=torch.long, device=dev)
                eps = noise.get("plan_eps")
                eps = None if eps is None else eps.to(dev, torch.float32).reshape(R, -1).index_select(0, nidx)
                ce = noise.get("cem_eps")
                ce = None if ce is None else ce.to(dev, torch.float32).index_select(0, nidx)
                if embeddings is not None:
                    src = self._source_embedded(embeddings, nidx, eps, ce)
                else:
                    src = self._source(observation, goal, nidx, eps, ce)
                src = src.to(torch.float32).reshape(len(need), -1)
                new = src if need == due else torch.zeros(R, self.ad.P, device=dev).index_copy_(0, nidx, src).index_select(0, idx)
            if plans is not None:
                given_rows = plans.to(dev, torch.float32).reshape(R, -1).index_select(0, idx)
                if new is None:
                    new = given_rows
                else:
                    new = torch.where(torch.isnan(given_rows).any(dim=1, keepdim=True), new, given_rows)
            self.plan.index_copy_(0, idx, new)
        if embeddings is not None:
            emb = _cat_rows(embeddings.obs["lmp"], self.module.action_decoder_modalities)
        elif self.image:
            emb = self.module.perceptual_encoder.get_state_from_observation(
                observation=observation, modalities=self.module.action_decoder_modalities)
        else:
            emb = observation
        restart = [False] * R
        for r in due:
            restart[r] = True
        draws = None
        if "rand_a" in noise or "rand_b" in noise:
            ra, rb = noise.get("rand_a"), noise.get("rand_b")
            draws = (ra if ra is not None else torch.rand(R, self.ad.Da, self.ad.K, device=dev),
                     rb if rb is not None else torch.rand(R, self.ad.Da, device=dev))
        out = self.ad.step_rows(self.state, self.plan, emb.contiguous(), restart, noise=draws)
        self.clock.tick(set(due))
        return out


def default_batch_obs(raw, envs):
    """Vector environments (rollout_manager_d4rl.py:126-135): the stacked observations and each environment's goal -
    `target_goal`, or `goal_locations[0]`."""
    goals = [env.target_goal if hasattr(env, "target_goal") else env.goal_locations[0] for env in envs]
    return (torch.as_tensor(np.stack([np.asarray(o, dtype=np.float32) for o in raw])),
            torch.as_tensor(np.stack([np.asarray(g, dtype=np.float32) for g in goals])))


def rollout_episodes(policy, envs, max_steps=None, batch_obs=None, noise=None, reset_infos=None, ingest=None, actions_out=None):
    """One episode per environment, all at once: envs is a list of policy.R gym-API objects (`reset()`, `step(a)` ->
    (obs, reward, done, info), `_max_episode_steps`).  One `.cpu()` of the (R, A) actions per step; finished rows idle (their
    last observation is fed again, their actions are dropped).  batch_obs(list of raw observations, envs) -> (observation,
    goal) for policy.step; noise: None or a callable step -> the step's noise dict.
    reset_infos: None or one dict per environment, passed as `env.reset(**reset_info)` (rollout_manager.py:111, :216).
    ingest: None or a FrameIngest of R rows, used in place of batch_obs: the raw uint8 frames become the step's
    `embeddings=`; its goal cache is dropped with the policy's reset.  actions_out: None or a list that receives, per
    environment, the list of the actions it was stepped with.
    Returns the reference's rollout_info dicts (`episode_length`, `episode_return`, `success`, and `successful_tasks` where
    the environment's last info reports it, :177-178), one per environment."""
    R = len(envs)
    if R != policy.R:
        raise ValueError(f"{R} environments for a policy of {policy.R} rows")
    if reset_infos is not None and len(reset_infos) != R:
        raise ValueError(f"{len(reset_infos)} reset_infos for {R} environments")
    if ingest is not None and ingest.R != R:
        raise ValueError(f"{R} environments for an ingest of {ingest.R} rows")
    batch_obs = batch_obs or default_batch_obs
    raw = [env.reset(**(reset_infos[r] if reset_infos is not None else {})) for r, env in enumerate(envs)]
    policy.reset()
    if ingest is not None:
        ingest.reset()
    limit = [env._max_episode_steps if max_steps is None else min(max_steps, env._max_episode_steps) for env in envs]
    steps, returns, info = [0] * R, [0] * R, [{} for _ in range(R)]
    live = [limit[r] > 0 for r in range(R)]
    if actions_out is not None:
        actions_out[:] = [[] for _ in range(R)]
    t = 0
    while any(live):
        step_noise = noise(t) if noise is not None else None
        if ingest is not None:
            actions = policy.step(None, None, noise=step_noise, embeddings=ingest.step(raw))
        else:
            observation, goal = batch_obs(raw, envs)
            actions = policy.step(observation, goal, noise=step_noise)
        actions = actions.cpu().numpy()
        for r in range(R):
            if not live[r]:
                continue
            if actions_out is not None:
                actions_out[r].append(actions[r].copy())
            raw[r], reward, done, info[r] = envs[r].step(actions[r])
            returns[r] += reward
            steps[r] += 1
            live[r] = not (done or steps[r] >= limit[r])
        t += 1
    out = []
    for r in range(R):
        d = {"episode_length": steps[r], "episode_return": returns[r], "success": ("success" in info[r]) and info[r]["success"]}
        if "successful_tasks" in info[r]:
            d["successful_tasks"] = info[r]["successful_tasks"]
        out.append(d)
    return out


def rollout_episodes_refill(policy, envs, episodes, noise=None, ingest=None, max_steps=None, batch_obs=None, actions_out=None,
                            refill=True):
    """A queue of episodes over the R = len(envs) = policy.R slots: episodes is a list of (key, reset_info), possibly longer
    than R.  The first min(R, n) start in slots 0, 1, 2, ...; when a row's episode ends (`done`, or its step count reaches the
    limit of rollout_episodes) its rollout_info is stored at the episode's position and - the queue not empty - the slot takes
    the next episode on the following step: `env.reset(**reset_info)`, `policy.reset(rows=[r])`, `ingest.reset(rows=[r])`, the
    row's step counter back to 0 (PlanClock re-plans a row on its first step after its reset).  Rows idle only when the queue
    is empty (their last observation is fed again, their actions are dropped); with fewer episodes than slots the spare rows
    idle from the start, on slot 0's first observation.
    refill=False: a slot waits until every row is done, then all slots take the next R episodes at once - the same episodes in
    fixed batches, for comparison.
    noise: None or a callable (keys, steps, due_rows) -> the step's noise dict for policy.step - keys[r] / steps[r]: the key
    and the step counter of the episode in row r (an idle row keeps its last ones; None / 0 for a row that never ran);
    due_rows: the running rows that re-plan on this step (every running row for a policy without a clock).
    Returns the rollout_info dicts of rollout_episodes in episode order; actions_out receives each episode's action list."""
    R, n = len(envs), len(episodes)
    if n == 0:
        raise ValueError("no episodes to run")
    if R != policy.R:
        raise ValueError(f"{R} environments for a policy of {policy.R} rows")
    if ingest is not None and ingest.R != R:
        raise ValueError(f"{R} environments for an ingest of {ingest.R} rows")
    batch_obs = batch_obs or default_batch_obs
    clock = getattr(policy, "clock", None)
    out = [None] * n
    if actions_out is not None:
        actions_out[:] = [[] for _ in range(n)]
    raw, keys, ep = [None] * R, [None] * R, [None] * R  # ep[r]: the position of the row's running episode, None: idle
    steps, returns, limit, info = [0] * R, [0] * R, [0] * R, [{} for _ in range(R)]
    queue = 0

    def finish(r):
        d = {"episode_length": steps[r], "episode_return": returns[r], "success": ("success" in info[r]) and info[r]["success"]}
        if "successful_tasks" in info[r]:
            d["successful_tasks"] = info[r]["successful_tasks"]
        out[ep[r]] = d
        ep[r] = None

    def start(r):
        nonlocal queue
        keys[r], reset_info = episodes[queue]
        ep[r], queue = queue, queue + 1
        raw[r] = envs[r].reset(**(reset_info or {}))
        steps[r], returns[r], info[r] = 0, 0, {}
        limit[r] = envs[r]._max_episode_steps if max_steps is None else min(max_steps, envs[r]._max_episode_steps)
        if limit[r] <= 0:
            finish(r)

    def fill_slots():
        new = []
        for r in range(R):
            while ep[r] is None and queue < n:
                start(r)
                new.append(r)
        return sorted(set(new))

    fill_slots()
    for r in range(R):
        if raw[r] is None:  # more slots than episodes: a spare row is fed slot 0's first observation, its environment untouched
            raw[r] = raw[0]
    policy.reset()
    if ingest is not None:
        ingest.reset()
    while any(e is not None for e in ep):
        running = [r for r in range(R) if ep[r] is not None]
        if noise is not None:
            due = running if clock is None else [r for r in clock.due() if ep[r] is not None]
            step_noise = noise(list(keys), list(steps), due)
        else:
            step_noise = None
        if ingest is not None:
            actions = policy.step(None, None, noise=step_noise, embeddings=ingest.step(raw))
        else:
            observation, goal = batch_obs(raw, envs)
            actions = policy.step(observation, goal, noise=step_noise)
        actions = actions.cpu().numpy()
        for r in running:
            if actions_out is not None:
                actions_out[ep[r]].append(actions[r].copy())
            raw[r], reward, done, info[r] = envs[r].step(actions[r])
            returns[r] += reward
            steps[r] += 1
            if done or steps[r] >= limit[r]:
                finish(r)
        if refill or all(e is None for e in ep):
            new = fill_slots()
            if new:
                policy.reset(rows=new)
                if ingest is not None:
                    ingest.reset(rows=new)
    return out


def latent_plan_policy_restatement(plan_fn, decoder_fn, observations, goals, n_envs, plan_duration, hidden0, resets=None,
                                   plans=None):
    """LatentPlanPolicy's schedule in plain torch ops, over callables standing in for the networks (any device, any dtype).
      plan_fn(observation rows, goal rows, rows (list), t) -> (len(rows), P): the plan source, called with the rows that
        re-plan at step t only;
      decoder_fn(plan (R,P), observation (R,..), hidden, t) -> (actions (R,A), new hidden): one decoder step, `hidden` with
        the row dimension at index -2 (nn.RNN's (L, R, H));
      observations[t], goals[t]: the step's inputs; hidden0: zeros of the hidden state's shape;
      resets: {t: rows} - `reset(rows)` called BEFORE step t (t = 0 resets every row anyway);
      plans: {t: (R,P)} with NaN rows meaning "not given".
    Returns dict(actions [T x (R,A)], replanned [T x list of rows], plan [T x (R,P)], hidden (after the last step))."""
    clock = PlanClock(n_envs, plan_duration)
    hidden, plan = hidden0.clone(), None
    out = dict(actions=[], replanned=[], plan=[])
    for t in range(len(observations)):
        if resets and t in resets:
            clock.reset(resets[t])
        obs, goal = observations[t], goals[t]
        due = clock.due()
        for r in due:
            given = plans is not None and t in plans and not bool(torch.isnan(plans[t][r]).any())
            row = plans[t][r] if given else plan_fn(obs[r: r + 1], goal[r: r + 1], [r], t)[0]
            if plan is None:
                plan = torch.zeros(n_envs, row.shape[-1], dtype=row.dtype, device=row.device)
            plan = plan.clone()
            plan[r] = row
            hidden = hidden.clone()
            hidden[..., r, :] = 0  # clear_hidden_state(): the row starts from h_0 = 0
        actions, hidden = decoder_fn(plan, obs, hidden, t)
        clock.tick(set(due))
        out["actions"].append(actions)
        out["replanned"].append(due)
        out["plan"].append(plan.clone())
    out["hidden"] = hidden
    return out


# ------------------------------------------------------------------------------------------ relay imitation learning
class RelayPolicy:
    """The relay-imitation rollout (reference evaluation/rollout_manager.py:480-510) for R environments in one step:

        policy = RelayPolicy(module, n_envs=R, plan_duration=16)
        policy.reset(rows=None)
        actions = policy.step(observation, goal)                 # {camera: (R,3,H,W)} dicts -> (R, A) fp32 on the device
        actions = policy.step_embeddings(obs_emb, goal_emb)      # {camera: (R,32)} dicts in, the same out

    No recurrent state: every `plan_duration` steps, per row, the high-level policy turns [enc(obs) | goal_encoder(enc(goal))]
    into the latent sub-goal tanh(mean); on every step the low-level policy turns [enc(obs) | sub-goal] into tanh(mean) and an
    arg-max gripper bit.  The clock is PlanClock's host integers; nothing is read back from the device.  Each chain is ONE
    tacorl_rows_mlp_fwd call (route "rows") up to ROWS_KERNEL_MAX_R rows and the training chain plus the sampling kernel
    (route "composed") above it (profiles/ril_rollout.md); fp32 from the masters whatever the module's compute dtype.
    Nothing is captured in a hipGraph."""

    # profiles/ril_rollout.md: the rows chain is the faster route at every R measured (1 .. 64), so every row count a policy can
    # have takes it; a lower value set on an instance sends the chains above it through the composed route
    ROWS_KERNEL_MAX_R = 64
    MAX_ENVS = 64

    def __init__(self, module, n_envs, plan_duration=16):
        nets = getattr(module, "__dict__", {}).get("_rollout_nets")
        for name in ("high_level_policy", "low_level_policy"):
            if getattr(getattr(module, name, None), "get_actions", None) is None:
                raise ValueError(f"the module has no {name}.get_actions")
        if nets is None:
            raise ValueError("the module has no relay-imitation rollout surface")
        if not 1 <= int(n_envs) <= self.MAX_ENVS:
            raise ValueError(f"n_envs {n_envs}: 1 .. {self.MAX_ENVS}")
        from ..modules.inference import RowsMLP

        self.module, self.R, self.dev = module, int(n_envs), module.dev
        self.clock = PlanClock(n_envs, plan_duration)
        self.plan_duration = int(plan_duration)
        self.high_cams, self.low_cams = list(module.high_level_policy_modalities), list(module.low_level_policy_modalities)
        self.cams = list(self.low_cams)  # the union (each list is a permutation of it)
        g, hi, lo = nets["goal_encoder"], nets["high"], nets["low"]
        self.Eo, self.GO, self.A = 32 * len(self.cams), g.G, lo.A
        self.E = self.Eo + self.GO
        R = self.R
        self.genc = RowsMLP(module, g.genc, g.genc_dims, g.genc_acts, R)
        self.high = RowsMLP(module, hi.head, hi.head_dims, hi.head_acts, R, policy=(hi.Ac, hi.dg))
        self.low = RowsMLP(module, lo.head, lo.head_dims, lo.head_acts, R, policy=(lo.Ac, lo.dg))
        f = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
        self.ld = (self.E + 3) // 4 * 4  # rows of whole 16-byte words, pad columns zero (the composed route's vector loads)
        self.gin, self.hin, self.lin = f(R, self.Eo), f(R, self.ld), f(R, self.ld)
        self.hout, self.subgoal, self.actions = f(R, self.GO), f(R, self.GO), f(R, self.A)
        self._rows_ok = {}  # row count -> tacorl_rows_mlp_supported, asked once

    def reset(self, rows=None):
        """All rows, or an index list / bool mask: those rows get a new sub-goal on their next step."""
        self.clock.reset(rows)

    def rows_route(self, n):
        """'rows' (tacorl_rows_mlp_fwd) or 'composed' (ops.mlp_fwd + ops.tanh_normal_sample) for a chain of n rows."""
        if n not in self._rows_ok:
            self._rows_ok[n] = self.low.supported(n)
        return "rows" if n <= self.ROWS_KERNEL_MAX_R and self._rows_ok[n] else "composed"

    # ------------------------------------------------------------------ the two halves of a step
    def replan(self, obs_rows, goal_rows, n, route=None):
        """Sub-goals of n rows: obs_rows / goal_rows {camera: (n,32)} -> self.hout[:n] (a view)."""
        route = route or self.rows_route(n)
        for j, c in enumerate(self.high_cams):
            self.gin[:n, 32 * j: 32 * j + 32] = goal_rows[c]
            self.hin[:n, 32 * j: 32 * j + 32] = obs_rows[c]
        self.genc.run(self.gin, self.Eo, n, self.hin, self.Eo, self.ld, route)
        self.high.run(self.hin, self.ld, n, self.hout, 0, self.GO, route)
        return self.hout[:n]

    def decode(self, obs_emb, route=None):
        """The low-level chain over all R rows on [state in low order | self.subgoal] -> self.actions."""
        for j, c in enumerate(self.low_cams):
            self.lin[:, 32 * j: 32 * j + 32] = obs_emb[c]
        self.lin[:, self.Eo: self.E] = self.subgoal
        self.low.run(self.lin, self.ld, self.R, self.actions, 0, self.A, route or self.rows_route(self.R))
        return self.actions

    def _advance(self, obs_emb, goal_rows_of, subgoals):
        R, dev = self.R, self.dev
        due = self.clock.due()
        if due:
            need = due
            if subgoals is not None and not subgoals.is_cuda:  # a host tensor: which rows it gives is known without a device read
                given = (~torch.isnan(subgoals.reshape(R, -1)).any(dim=1)).tolist()
                need = [r for r in due if not given[r]]
            idx = torch.tensor(due, dtype=torch.long, device=dev)
            new = None
            if need:
                nidx = idx if need == due else torch.tensor(need, dtype=torch.long, device=dev)
                src = self.replan(_take(obs_emb, nidx), goal_rows_of(nidx), len(need))
                new = src if need == due else torch.zeros(R, self.GO, device=dev).index_copy_(0, nidx, src).index_select(0, idx)
            if subgoals is not None:
                given_rows = subgoals.to(dev, torch.float32).reshape(R, -1).index_select(0, idx)
                new = given_rows if new is None else torch.where(torch.isnan(given_rows).any(dim=1, keepdim=True), new, given_rows)
            self.subgoal.index_copy_(0, idx, new)
        out = self.decode(obs_emb)
        self.clock.tick(set(due))
        return out

    def step_embeddings(self, obs_emb, goal_emb, subgoals=None):
        """obs_emb / goal_emb: {camera: (R,32)} state embeddings of every camera of the union.  subgoals: (R, goal_out) with NaN
        rows meaning "not given" - overrides the high-level policy for the rows that are due.  Returns the (R, A) actions: a
        view that stays valid until the next step."""
        to = lambda d: {c: torch.as_tensor(d[c]).to(self.dev, torch.float32) for c in self.cams}  # noqa: E731
        obs_emb, goal_emb = to(obs_emb), to(goal_emb)
        return self._advance(obs_emb, lambda nidx: _take(goal_emb, nidx), subgoals)

    def step(self, observation, goal, noise=None, subgoals=None, embeddings=None):
        """observation / goal: {camera: (R,3,H,W)} fp32 dicts.  Every camera of the union is encoded once for all R rows; the
        goal images of the rows that are due only.  noise is accepted for rollout_episodes and unused (the actions are
        deterministic).  embeddings: a FrameIngest step's result in place of the two image dicts."""
        if embeddings is not None:
            return self._advance(embeddings.obs["ril"], lambda nidx: _take(embeddings.goal["ril"], nidx), subgoals)
        to = lambda d: {c: torch.as_tensor(d[c]).to(self.dev, torch.float32) for c in self.cams}  # noqa: E731
        observation, goal = to(observation), to(goal)
        pe = self.module.perceptual_encoder
        obs_emb = pe.get_state_from_observation(observation=observation, modalities=self.cams, cat_output=False)
        goal_rows = lambda nidx: pe.get_state_from_observation(  # noqa: E731
            observation=_take(goal, nidx), modalities=self.cams, cat_output=False)
        return self._advance(obs_emb, goal_rows, subgoals)


def relay_policy_restatement(high_fn, low_fn, obs_embs, goal_embs, n_envs, plan_duration, resets=None, subgoals=None):
    """RelayPolicy's schedule in plain torch ops, over callables standing in for the networks (any device, any dtype).
      high_fn(obs rows {camera: (1,32)}, goal rows {camera: (1,32)}, rows (list), t) -> (len(rows), GO): the sub-goal of the
        rows that are due at step t - goal encoder and high-level policy;
      low_fn(obs {camera: (R,32)}, sub-goal (R,GO), t) -> (R,A): one low-level step over all rows;
      obs_embs[t], goal_embs[t]: the step's per-camera embeddings;
      resets: {t: rows} - `reset(rows)` called BEFORE step t (t = 0 resets every row anyway);
      subgoals: {t: (R,GO)} with NaN rows meaning "not given".
    Returns dict(actions [T x (R,A)], replanned [T x list of rows], subgoal [T x (R,GO)])."""
    clock = PlanClock(n_envs, plan_duration)
    sub = None
    out = dict(actions=[], replanned=[], subgoal=[])
    for t in range(len(obs_embs)):
        if resets and t in resets:
            clock.reset(resets[t])
        obs, goal = obs_embs[t], goal_embs[t]
        due = clock.due()
        for r in due:
            given = subgoals is not None and t in subgoals and not bool(torch.isnan(subgoals[t][r]).any())
            row = subgoals[t][r] if given else high_fn({c: v[r: r + 1] for c, v in obs.items()},
                                                       {c: v[r: r + 1] for c, v in goal.items()}, [r], t)[0]
            if sub is None:
                sub = torch.zeros(n_envs, row.shape[-1], dtype=row.dtype, device=row.device)
            sub = sub.clone()
            sub[r] = row
        out["actions"].append(low_fn(obs, sub, t))
        clock.tick(set(due))
        out["replanned"].append(due)
        out["subgoal"].append(sub.clone())
    return out


# ------------------------------------------------------------------------------------------ the flat baseline
class RLPolicy:
    """The RLRollout manager's inner loop (reference evaluation/rollout_manager.py:121-141) for R environments in one step:

        policy = RLPolicy(module, n_envs=R, use_cem=False)
        policy.reset(rows=None)                                  # nothing to forget: the policy has no state
        actions = policy.step(observation, goal)                 # (R, A) fp32 on the device

    `actor.get_actions(obs, deterministic=True, reparameterize=False)` on every row, every step - tanh(mean), and with a
    discrete gripper the arg-max class, as ActorSurface.get_actions states it - and with use_cem
    `CEMOptimizer.get_action(obs, initial_mean=that action)` over all R rows in its one launch, discrete_gripper taken from the
    actor as the manager does (:101-106).  Image modules (CQL_Offline) take {camera: (R,3,H,W)} dicts or `embeddings=`, vector
    modules (the D4RL CQL) (R,S) / (R,G) tensors."""

    def __init__(self, module, n_envs, use_cem=False, cem_kwargs=None):
        actor = getattr(module, "actor", None)
        if getattr(actor, "get_actions", None) is None:
            raise ValueError("the module has no actor.get_actions")
        if int(n_envs) < 1:
            raise ValueError(f"n_envs {n_envs}")
        self.module, self.R, self.dev, self.actor = module, int(n_envs), module.dev, actor
        self.image = hasattr(getattr(module, "__dict__", {}).get("_actor_surface"), "cams")
        self.A = int(actor.action_dim)
        self.cem = None
        if use_cem:
            from ..modules.cem import CEMOptimizer

            self.cem = CEMOptimizer(q1=module.q1, q2=module.q2, action_dim=self.A,
                                    discrete_gripper=bool(actor.discrete_gripper), **(cem_kwargs or {}))

    def reset(self, rows=None):
        _row_list(rows, self.R)

    def step(self, observation, goal=None, noise=None, embeddings=None):
        """noise: None or {"cem_eps": (R, iters, N, A)} - the CEM draws; the actor's action is deterministic."""
        dev, noise = self.dev, noise or {}
        if embeddings is not None:
            if not self.image:
                raise ValueError("embeddings= stands in for images: this module takes vector observations")
            surf = self.module.__dict__["_actor_surface"]
            o = _obs_goal_rows(self.module, surf.net, embeddings, "actor", surf.cams, surf.goal_cams)
            o_cem = _critic_rows(self.module, embeddings) if self.cem is not None else None
        else:
            to = lambda x: ({k: to(v) for k, v in x.items()} if isinstance(x, dict) else torch.as_tensor(x).to(dev, torch.float32))  # noqa: E731
            observation = to(observation)
            if goal is None:
                o = observation
            elif self.image:
                o = {"observation": observation, "goal": to(goal)}
            else:
                o = torch.cat([observation, to(goal)], dim=-1)
            o_cem = o
        actions, _ = self.actor.get_actions(o, deterministic=True, reparameterize=False)
        if self.cem is not None:
            eps = noise.get("cem_eps")
            actions = self.cem.get_action(obs=o_cem, initial_mean=actions, noise=None if eps is None else {"eps": eps})
        return actions


def rl_policy_restatement(actor_fn, observations, goals, n_envs, cem_fn=None):
    """RLPolicy's schedule in plain torch ops, over callables standing in for the networks (any device, any dtype).
      actor_fn(observation (R,..), goal (R,..) or None, t) -> (R, A): the deterministic action of every row;
      cem_fn(observation, goal, initial_mean (R,A), t) -> (R, A): the refinement (None: use_cem off);
      observations[t], goals[t] (or goals None): the step's inputs.
    Returns dict(actions [T x (R,A)], initial_mean [T x (R,A)])."""
    out = dict(actions=[], initial_mean=[])
    for t in range(len(observations)):
        obs, goal = observations[t], (goals[t] if goals is not None else None)
        a = actor_fn(obs, goal, t)
        if a.shape[0] != n_envs:
            raise ValueError(f"{a.shape[0]} action rows for {n_envs} environments")
        out["initial_mean"].append(a)
        out["actions"].append(cem_fn(obs, goal, a, t) if cem_fn is not None else a)
    return out
