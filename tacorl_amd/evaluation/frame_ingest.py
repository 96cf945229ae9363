"""From the environments' raw camera frames to what a rollout policy's step consumes (reference evaluation/rollout_manager.py:
`transform_observation(..., transf_type="validation")` in front of every network call, utils/transforms.py:333-348):

    ingest = FrameIngest(module, n_envs=R, transform_manager_cfg=cfg)
    ingest.reset(rows=None)                      # those rows' goal embeddings are computed again on their next step
    emb = ingest.step(raw)                       # raw: one observation per environment
                                                 # (= encode(submit()) behind stage(raw): the host half and the device half)
    actions = policy.step(None, None, embeddings=emb)

An observation is `{camera: uint8 (H_s, W_s, 3)}` or `{"observation": {camera: ...}, "goal": {camera: ...}}`, at whatever
resolution the environment renders.  Per step and camera the R frames (and the goal frames of the rows whose episode has just
begun) go into one pinned uint8 staging buffer and cross in ONE copy; the validation list of the transform manager - Resize ->
ScaleImageTensor -> Normalize(0.5, 0.5), read by data/augment.py's augment_specs, which refuses what it refuses for a
datamodule - is tacorl_resize_frames_u8 followed by the uint8 pack, the two launches a resident replay's validation batch
goes through (data/resident.py: store_size, then tacorl_pack_images_u8*): the packed images are that batch's, bit for bit.
All (network, camera) encoder problems of the step - every network's encoders over the observations, the goal cameras of the
rows that need them - are then handed to encoder_stage.encode: one fused launch per camera geometry where fused_fwd_ok
holds (packed conv weights kept current by PackedWeights' version rule), the per-layer entry point otherwise.

The goal is constant over an episode: its embeddings are computed on a row's first step after `reset` and kept per row.
Nothing is read back from the device, nothing is captured in a hipGraph, and no buffer a captured training step knows is
touched."""
import numpy as np
import torch

from .. import encoder_stage as stage
from .. import ops
from ..data.augment import augment_specs


class StepEmbeddings:
    """obs[network][camera]: (R,32) embeddings of this step's observations; goal[network][camera]: (R,32), each row the
    embedding of that row's goal since its last reset.  Views of the ingest's buffers: valid until its next step."""

    def __init__(self, obs, goal):
        self.obs, self.goal = obs, goal


def ingest_networks(module, use_cem=False):
    """The encoder networks a rollout of `module` runs, as [(name, parameter block, observation cameras, goal cameras)]:
    "actor" (CQL_Offline, TACORL: the actor's own encoders), "lmp" (PlayLMP, TACORL: the perceptual encoder that feeds the plan
    proposal and the action decoder), "ril" (RelayImitationLearning: the shared encoders) and, under use_cem, "q1" (the critic
    CEMOptimizer maximises over)."""
    d = getattr(module, "__dict__", {})
    if d.get("_rollout_nets") is not None:
        blk = module.engine.blk
        return [("ril", blk, list(module.low_level_policy_modalities), list(module.low_level_policy_modalities))]
    surf = d.get("_actor_surface")
    if surf is None or not hasattr(surf, "cams"):
        raise ValueError(f"{type(module).__name__} has no image rollout surface (vector observations need no ingest)")
    nets = []
    if getattr(getattr(module, "actor", None), "get_actions", None) is not None:
        nets.append(("actor", surf.net, list(surf.cams), list(surf.goal_cams)))
        lmp = d.get("lmp_net", getattr(module, "lmp_net", None))
        if lmp is not None:
            nets.append(("lmp", lmp, list(module.action_decoder_modalities), []))
        if use_cem:
            cs = module.q1.__dict__["critic_surface"]
            nets.append(("q1", cs.net, list(cs.cams), list(cs.goal_cams)))
    else:  # PlayLMP: one network block behind plan proposal, goal encoder and action decoder
        obs = list(dict.fromkeys(list(module.plan_proposal_obs_modalities) + list(module.action_decoder_modalities)))
        nets.append(("lmp", surf.net, obs, list(module.plan_proposal_goal_modalities)))
    return nets


class FrameIngest:
    def __init__(self, module, n_envs, transform_manager_cfg=None, use_cem=False):
        if int(n_envs) < 1:
            raise ValueError(f"n_envs {n_envs}")
        self.nets = ingest_networks(module, use_cem)
        self.module, self.R, self.dev = module, int(n_envs), module.dev
        self.obs_cams = list(dict.fromkeys(c for _, _, oc, _ in self.nets for c in oc))
        self.goal_cams = list(dict.fromkeys(c for _, _, _, gc in self.nets for c in gc))
        self.cams = list(dict.fromkeys(self.obs_cams + self.goal_cams))
        specs = augment_specs(transform_manager_cfg, self.cams, "validation")  # (raises for what is not built)
        for c, sp in specs.items():
            if sp is not None and (sp.pad or sp.prob):
                raise NotImplementedError(f"{c}: the validation list draws an augmentation; a rollout's transform is Resize, "
                                          "ScaleImageTensor and Normalize(0.5, 0.5)")
        self.resize = {c: (sp.resize if sp is not None else None) for c, sp in specs.items()}
        self.compute, self.img_dtype = module.compute, module.img_dtype
        self.packs = stage.PackedWeights(self.dev)
        self.goal_valid = [False] * self.R
        self.src_hw, self.hw, self._buf = {}, {}, None
        self._copied = None
        self.launches = {}  # entry point -> calls of the last step (tools/time_rollout_ingest.py reads it)

    # ------------------------------------------------------------------ rows
    def reset(self, rows=None):
        """All rows, or an index list / bool mask: those rows' goal embeddings are computed again on their next step."""
        from .vec_policy import _row_list

        for r in _row_list(rows, self.R):
            self.goal_valid[r] = False

    # ------------------------------------------------------------------ buffers
    def _allocate(self, frames):
        """frames: {camera: one uint8 (Hs, Ws, 3) frame} - the geometry every later frame of that camera must have."""
        R, dev = self.R, self.dev
        esz = 2 if self.img_dtype == torch.bfloat16 else 4
        b = dict(stage={}, stage_np={}, raw={}, small={}, img={}, img_bytes={}, out={}, gout={}, cache={}, act={}, gact={})
        for c in self.cams:
            f = np.asarray(frames[c])
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise TypeError(f"{c}: a frame is uint8 (H, W, 3), got {f.dtype} {f.shape}")
            Hs, Ws = int(f.shape[0]), int(f.shape[1])
            H, W = self.resize[c] or (Hs, Ws)
            if (H * W * 3) % 16:
                raise NotImplementedError(f"{c}: the uint8 pack takes images of a multiple of 16 bytes, {H}x{W}x3 is not")
            self.src_hw[c], self.hw[c] = (Hs, Ws), (H, W)
            b["stage"][c] = torch.zeros(2 * R, Hs, Ws, 3, dtype=torch.uint8).pin_memory()
            b["stage_np"][c] = b["stage"][c].numpy()
            b["raw"][c] = torch.zeros(2 * R, Hs, Ws, 3, dtype=torch.uint8, device=dev)
            b["small"][c] = b["raw"][c] if (H, W) == (Hs, Ws) else torch.zeros(2 * R, H, W, 3, dtype=torch.uint8, device=dev)
            b["img"][c] = torch.zeros(2 * R, H, W, 3, dtype=self.img_dtype, device=dev)
            b["img_bytes"][c] = H * W * 3 * esz
        z = lambda: torch.zeros(R, 32, device=dev)  # noqa: E731
        for name, _, oc, gc in self.nets:
            b["out"][name], b["gout"][name], b["cache"][name] = {c: z() for c in oc}, {c: z() for c in gc}, {c: z() for c in gc}
            n_act = lambda c: ops.encoder_act_layout(R, *self.hw[c])[1]  # noqa: E731
            fused = lambda c: stage.fused_fwd_ok(self.hw[c], self.compute, self.img_dtype)  # noqa: E731
            # (saved activations are the per-layer entry point's workspace; the fused forward of a rollout saves none)
            b["act"][name] = {c: None if fused(c) else torch.zeros(n_act(c), device=dev) for c in oc}
            b["gact"][name] = {c: None if fused(c) else torch.zeros(n_act(c), device=dev) for c in gc}
        self._buf = b
        self._copied = torch.cuda.Event()

    # ------------------------------------------------------------------ one step
    def _split(self, raw):
        """Per environment (observation frames, goal frames or None)."""
        out = []
        for o in raw:
            if isinstance(o, dict) and "goal" in o:
                out.append((o["observation"], o["goal"]))
            else:
                out.append((o, None))
        return out

    def stage(self, raw):
        """The host half of a step: the frames into the pinned staging buffers.  Returns the rows whose goal frames went with
        them (`submit` issues the device half)."""
        R = self.R
        if len(raw) != R:
            raise ValueError(f"{len(raw)} observations for an ingest of {R} rows")
        pairs = self._split(raw)
        g_rows = [r for r in range(R) if not self.goal_valid[r]] if self.goal_cams else []
        for r in g_rows:
            if pairs[r][1] is None:
                raise ValueError(f"row {r}: the networks take a goal, the observation must be {{'observation': ..., 'goal': ...}}")
        if self._buf is None:
            first = dict(pairs[0][0])
            if pairs[0][1] is not None:
                first.update({c: pairs[0][1][c] for c in self.goal_cams if c not in first})
            missing = [c for c in self.cams if c not in first]
            if missing:
                raise KeyError(f"the observation has no frame of {missing}")
            self._allocate(first)
        b, k = self._buf, len(g_rows)
        self._copied.synchronize()  # the previous step's copies have left the staging buffers
        self._staged = (g_rows, {})
        for c in self.cams:
            is_obs, is_goal = c in self.obs_cams, c in self.goal_cams and k > 0
            lo, hi = (0 if is_obs else R), (R + k if is_goal else R)
            if lo == hi:
                continue
            st = b["stage_np"][c]
            want = self.src_hw[c] + (3,)
            put = []
            if is_obs:
                put += [(r, pairs[r][0][c]) for r in range(R)]
            if is_goal:
                put += [(R + i, pairs[r][1][c]) for i, r in enumerate(g_rows)]
            for row, f in put:
                f = np.asarray(f)
                if f.dtype != np.uint8 or f.shape != want:
                    raise TypeError(f"{c}: a frame is uint8 {want}, got {f.dtype} {f.shape}")
                st[row] = f
            self._staged[1][c] = (lo, hi)
        return g_rows

    def submit(self):
        """The device half of a staged step: per camera one copy and one resize, then one pack launch per geometry.  The packed
        images are self.images(camera): rows [0, R) the observations, rows [R, R + k) the k staged rows' goals."""
        b = self._buf
        g_rows, ranges = self._staged
        count = lambda name: self.launches.__setitem__(name, self.launches.get(name, 0) + 1)  # noqa: E731
        self.launches = {}
        jobs = {}
        for c, (lo, hi) in ranges.items():
            b["raw"][c][lo:hi].copy_(b["stage"][c][lo:hi], non_blocking=True)
            count("copy_h2d")
            if b["small"][c] is not b["raw"][c]:
                ops.resize_frames_u8(b["raw"][c][lo:hi], b["small"][c][lo:hi])
                count("tacorl_resize_frames_u8")
            H, W = self.hw[c]
            jobs.setdefault((H, W), []).append((b["small"][c][lo:hi].data_ptr(), H * W * 3, b["img"][c][lo:hi].data_ptr(), hi - lo))
        self._copied.record()
        for (H, W), js in jobs.items():
            ops.pack_images_u8_batch(js, stage.image_flag(self.img_dtype), H, W)
            count("tacorl_pack_images_u8_batch")
        return g_rows

    def pack(self, raw):
        """Stage, copy, resize and pack the step's frames; returns the rows whose goal frames went with them."""
        self.stage(raw)
        return self.submit()

    def images(self, cam):
        """The packed NHWC images of `cam`: (2R, H, W, 3) in the module's image dtype."""
        return self._buf["img"][cam]

    def _problems(self, cam, k):
        """The encoder problems of one camera: per network over its R observations, and over the k staged goals."""
        b, R = self._buf, self.R
        img = b["img"][cam].data_ptr()
        pr = []
        for name, blk, oc, gc in self.nets:
            if cam in oc:
                pr.append((img, blk, b["out"][name][cam], b["act"][name][cam], R, False, cam))
            if cam in gc and k > 0:
                pr.append((img + R * b["img_bytes"][cam], blk, b["gout"][name][cam], b["gact"][name][cam], k, False, cam))
        return pr

    def step(self, raw):
        """raw: R observations.  Returns the step's StepEmbeddings."""
        return self.encode(self.pack(raw))

    def encode(self, g_rows):
        """Every encoder problem of the packed step; g_rows: what `pack` / `submit` returned."""
        b, k = self._buf, len(g_rows)
        fused = lambda c: stage.fused_fwd_ok(self.hw[c], self.compute, self.img_dtype)  # noqa: E731
        cams = [c for c in self.cams if self._problems(c, k)]
        groups = stage.geometry_groups(cams, self.hw, fused, lambda c: len(self._problems(c, k)), stage.EF_MAXP)

        def launch(c, pr):
            for i in range(0, len(pr), stage.EF_MAXP):
                stage.launch_fused(pr[i: i + stage.EF_MAXP], self.packs, self.hw[c])
                self.launches["tacorl_encoder_fwd_fused_wg"] = self.launches.get("tacorl_encoder_fwd_fused_wg", 0) + 1

        stage.encode(groups, lambda c: self._problems(c, k), self.hw, self.compute, self.img_dtype, self.packs, fused,
                     lambda c: True, launch, pack_per_camera=False)
        if k:
            gidx = torch.tensor(g_rows, dtype=torch.long, device=self.dev)
            for name, _, _, gc in self.nets:
                for c in gc:
                    b["cache"][name][c].index_copy_(0, gidx, b["gout"][name][c][:k])
            for r in g_rows:
                self.goal_valid[r] = True
        return StepEmbeddings({name: b["out"][name] for name, *_ in self.nets}, {name: b["cache"][name] for name, *_ in self.nets})
