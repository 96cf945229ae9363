"""The data path of RelayImitationLearning (`experiment=relay_imitation_learning`): the sampling of the reference's RILDataset
(datamodule/dataset/relay_imitation_learning_dataset.py:73-113,181-206) as index arithmetic with explicit draws (RelayIndex),
the uint8 dataset resident in HBM with one sampler launch per batch (HbmRelayReplay, `tacorl_sample_relay`), and the loader /
datamodule that `Trainer.fit` takes (RelayLoader, RILDataModule - the counterpart of the reference's
datamodule/basic_data_module.py BasicDataModule with the RILDataset config).  The reference reads four .npz frames per item
from disk; here a batch is four frame ids per sample, and the module's image pack reads the frames by id.
"""
import numpy as np
import torch

from .. import ops
from .augment import AugmentSpec, RIL_ROLES, draw_ril_batch_augmentation

SLOTS = RIL_ROLES  # the four image roles of an item, in the order of the id table's rows (the RIL engine's image slots)


class RelayIndex:
    """RILDataset.__getitem__ as a deterministic function of explicit draws, as TransitionIndex is for the transitions.  With
    Lw = max_low_level_window, Hw = max_high_level_window and step = episode_lookup[idx] in the episode that ends at `end`:

        sub  = min(end, step + Lw)                                   high_level_action, the subgoal frame
        low  = step + 1 + floor(u_low * (sub - step - 1))   if sub - step - 1 > 0 else sub      low_level_goal
        hmax = min(end, step + Hw)
        high = sub + floor(u_high * (hmax - sub))           if hmax - sub > 0 else hmax         high_level_goal

    (sample_goal_step draws np.random.choice(np.arange(start, stop)) where the range is not empty - the upper bound is
    exclusive - and returns `stop` otherwise; hmax lies before sub when Hw < Lw), low_level_action = the action row of `step`.
    Items (load_file_indices): range(s, e + 1 - Lw) of every episode (s, e), none for an episode shorter than Lw + 1;
    len = int(len(items) * percentage), the first items, as BasicDataModule's Subset keeps them.
    tests/golden/relay_sampler.npz (recorded from the reference class) pins it; `tacorl_sample_relay` is the same arithmetic
    on the device.  The tables are validated here, once: every id the arithmetic can then produce lies in [0, n_frames) -
    step <= end - Lw, so step < low <= sub = step + Lw <= end and high <= max(sub, hmax) <= end - which is what the
    unchecked device gathers rely on."""

    def __init__(self, ep_start_end_ids, n_frames=None, max_low_level_window=30, max_high_level_window=260, percentage=1.0,
                 train=True):
        self.low_window, self.high_window, self.train = int(max_low_level_window), int(max_high_level_window), train
        if self.low_window < 1 or self.high_window < 1:
            raise ValueError(f"windows must be >= 1: low {self.low_window}, high {self.high_window}")
        if not 0.0 <= float(percentage) <= 1.0:
            raise ValueError(f"percentage {percentage} outside [0, 1]")
        self.ep = np.asarray(ep_start_end_ids, dtype=np.int64).reshape(-1, 2)
        if len(self.ep) == 0:
            raise ValueError("no episodes")
        self.n_frames = int(n_frames) if n_frames is not None else int(self.ep[:, 1].max()) + 1
        if self.ep.min() < 0 or self.ep.max() >= self.n_frames:
            raise ValueError(f"episode bounds outside [0, {self.n_frames})")
        if (self.ep[:, 0] > self.ep[:, 1]).any() or (self.ep[1:, 0] <= self.ep[:-1, 1]).any():
            raise ValueError("episodes must be sorted by start and must not overlap")
        if (self.ep[:, 1] <= self.low_window).any():  # the reference asserts on the absolute index (:201)
            raise ValueError(f"an episode ends at frame {int(self.ep[:, 1].min())} <= max_low_level_window {self.low_window}")
        look = np.concatenate([np.arange(s, max(e + 1 - self.low_window, s)) for s, e in self.ep]).astype(np.int64)
        self.episode_lookup = look[: int(len(look) * float(percentage))]
        if len(self.episode_lookup) == 0:
            raise ValueError("the index has no item (no episode longer than max_low_level_window, or percentage too small)")

    def __len__(self):
        return len(self.episode_lookup)

    def draw(self, n, rng):
        """The random quantities n items consume: the item and the uniforms of the two np.random.choice calls (:77)."""
        return {"idx": rng.integers(0, len(self), size=n).astype(np.int64), "u_low": rng.random(n), "u_high": rng.random(n)}

    def draw_device(self, n, device, generator=None):
        """`draw` made by torch on the device (nothing crosses PCIe): int64 idx, float64 u_low / u_high.  Items are drawn
        with replacement, as the other two feeders draw theirs; the reference's DataLoader(shuffle=True) draws WITHOUT
        replacement - every item once per epoch, in a random order."""
        dev, g = torch.device(device), generator
        return {"idx": torch.randint(0, len(self), (n,), device=dev, generator=g, dtype=torch.int64),
                "u_low": torch.rand(n, device=dev, generator=g, dtype=torch.float64),
                "u_high": torch.rand(n, device=dev, generator=g, dtype=torch.float64)}

    def episode_end(self, step):
        """find_episode_end (:115-119) by binary search: the end of the episode with start <= step <= end."""
        k = np.maximum(np.searchsorted(self.ep[:, 0], np.asarray(step), side="right") - 1, 0)
        return self.ep[k, 1]

    def sample(self, idx, d):
        """idx (n,) items (None: d["idx"]); d = draw(...).  Returns the four frame ids under the SLOTS names, `step`
        (= obs) and `idx`."""
        idx = np.asarray(d["idx"] if idx is None else idx, dtype=np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"item outside [0, {len(self)})")
        u_low, u_high = np.asarray(d["u_low"], dtype=np.float64), np.asarray(d["u_high"], dtype=np.float64)
        pick = lambda u, n: np.clip((u * n).astype(np.int64), 0, np.maximum(n - 1, 0))  # noqa: E731  floor(u n) in [0, n)
        step = self.episode_lookup[idx]
        end = self.episode_end(step)
        room = end - step
        sub = np.where(self.low_window >= room, end, step + np.minimum(self.low_window, room))  # min(end, step + Lw)
        hmax = np.where(self.high_window >= room, end, step + np.minimum(self.high_window, room))
        nl, nh = sub - step - 1, hmax - sub
        low = np.where(nl > 0, step + 1 + pick(u_low, np.maximum(nl, 0)), sub)
        high = np.where(nh > 0, sub + pick(u_high, np.maximum(nh, 0)), hmax)
        return {"obs": step, "low_level_goal": low, "high_level_goal": high, "high_level_action": sub, "step": step, "idx": idx}


class HbmRelayReplay:
    """RelayImitationLearning's batches out of a dataset resident in HBM: frames[cam] = (N,H,W,3) uint8, the (N,A) action
    table and the index tables all live on the device, and `batch()` is one launch of the sampler kernel
    (`tacorl_sample_relay`) on the current stream - no host synchronisation, nothing over PCIe.
    The returned tensors are views of this object's own buffers, a ring of `slots` sets (as HbmTransitionReplay's): a batch
    stays valid until `slots - 1` more have been drawn, so a trainer that fetches a batch or two ahead of the step it runs
    still trains on the batch it was given."""

    def __init__(self, frames, actions, index, device=None, batch_size=64, slots=6):
        self.dev = torch.device(device) if device is not None else next(iter(frames.values())).device
        self.index, self.batch_size = index, int(batch_size)
        self.frames = {c: torch.as_tensor(v).to(self.dev).contiguous() for c, v in frames.items()}
        acts = torch.as_tensor(np.asarray(actions, dtype=np.float32) if not torch.is_tensor(actions) else actions)
        acts = acts.to(self.dev, torch.float32).contiguous()
        short = [c for c, v in self.frames.items() if v.dtype != torch.uint8 or v.dim() != 4 or v.shape[0] < index.n_frames]
        if short or acts.dim() != 2 or acts.shape[0] < index.n_frames:
            raise ValueError(f"frames (uint8 (N,H,W,3)) and actions (N,A) must cover the index's {index.n_frames} frames")
        i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.dev)  # noqa: E731
        self.tables = {"lookup": i64(index.episode_lookup), "ep_start": i64(index.ep[:, 0]), "ep_end": i64(index.ep[:, 1]),
                       "actions": acts, "n_frames": index.n_frames}
        self.A = int(acts.shape[1])
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        self._cap, self._ring, self._k, self._u8 = 0, [{} for _ in range(int(slots))], 0, {}
        self._grow(self.batch_size)

    def _grow(self, B):
        """The batch buffers exist before the first batch and are replaced only for a larger one - under the capture lock,
        and captured graphs that could hold an old address are dropped (as HbmTransitionReplay._grow)."""
        if B <= self._cap:
            return
        with ops.capture_lock:
            for k in range(len(self._ring)):
                self._ring[k] = {"ids": torch.zeros(len(SLOTS) * B, dtype=torch.int64, device=self.dev),
                                 "action": torch.zeros(B * self.A, device=self.dev)}
            self._cap = B
            ops.note_alloc()

    def _out(self, key, shape):
        n = int(np.prod(shape))
        t = self._u8.get(key)
        if t is None or t.numel() < n:
            with ops.capture_lock:
                t = self._u8[key] = torch.empty(n, dtype=torch.uint8, device=self.dev)
                ops.note_alloc()
        return t[:n].view(shape)

    def check(self):
        """Reads the sampler's status word back (a host synchronisation: call it when you ask, not per step)."""
        if int(self.status.item()) != 0:
            raise IndexError("relay replay: the sampler had to clamp an id (tables or draws outside the dataset)")

    def batch(self, draws=None, aug=None, fused=True, batch_size=None):
        """draws: RelayIndex.draw_device(...) (None: drawn here for `batch_size`), or the host form `draw(...)`.
        fused=True: no frame moves here - the batch carries the dataset tensors and the (4, B) id table in SLOTS order
        (`batch["replay"]`), and RelayImitationLearning's image pack reads the frames by id on their way into the encoder.
        fused=False: the reference dataset's schema - the four role dicts of uint8 (B,H,W,3) frames gathered here
        (tacorl_gather_frames_u8) and `low_level_action`."""
        if draws is None:
            draws = self.index.draw_device(batch_size or self.batch_size, self.dev)
        d = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(self.dev).contiguous()
             for k, v in draws.items() if k in ("idx", "u_low", "u_high")}
        B = int(d["idx"].numel())
        self._grow(B)
        self._k = slot = (self._k + 1) % len(self._ring)
        buf = self._ring[slot]
        ids, act = buf["ids"][: len(SLOTS) * B].view(len(SLOTS), B), buf["action"][: B * self.A].view(B, self.A)
        ops.sample_relay(self.tables, d, self.index.low_window, self.index.high_window, ids, act, self.status)
        b = {"low_level_action": act}
        if aug is not None:
            b["aug"] = aug
        if fused:
            b["replay"] = {"kind": "relay", "frames": self.frames, "ids": ids, "B": B}
            return b
        for k, role in enumerate(SLOTS):
            b[role] = {c: ops.gather_frames_u8(fr, ids[k], self._out((slot, role, c), (B,) + tuple(fr.shape[1:])))
                       for c, fr in self.frames.items()}
        return b


class RelayLoader:
    """`steps_per_epoch` batches of `batch_size` fresh device draws per pass: what Trainer.fit takes as train_dataloaders /
    val_dataloaders for RelayImitationLearning.  train=False (validation) draws no augmentation.  A batch is views of the
    replay's ring of buffers (HbmRelayReplay(slots=6)): a trainer may hold up to `slots - 1` batches ahead of the one it runs."""

    def __init__(self, replay, batch_size, steps_per_epoch, aug_specs=None, generator=None, train=True, fused=True):
        self.replay, self.batch_size, self.steps_per_epoch = replay, int(batch_size), int(steps_per_epoch)
        self.aug_specs, self.generator, self.train, self.fused = aug_specs, generator, train, fused

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        rp = self.replay
        for _ in range(self.steps_per_epoch):
            draws = rp.index.draw_device(self.batch_size, rp.dev, self.generator)
            aug = None
            if self.train and self.aug_specs:
                aug = draw_ril_batch_augmentation(self.aug_specs, self.batch_size, rp.dev, self.generator)
            yield rp.batch(draws, aug=aug, fused=self.fused)


_DATASET_KEYS = ("max_low_level_window", "max_high_level_window", "path", "arrays")
_DATASET_UNUSED = ("_target_", "_recursive_", "modalities", "action_type", "n_digits", "transf_type")


def augment_specs(transform_manager, cams, split="train"):
    """{camera: AugmentSpec or None} out of a transform manager config of the `rl` form (config/datamodule/transform_manager/
    rl.yaml: transforms.<split>.<camera> = a list of {_target_, ...}): Resize(size) -> spec.resize, RandomShiftsAug(pad) ->
    spec.pad, ColorTransform(contrast, brightness, hue, prob) -> the spec's jitter; ScaleImageTensor and Normalize(0.5, 0.5)
    are what the uint8 pack computes anyway.  Any other transform of a camera in `cams` is not built.  None: no config."""
    if transform_manager is None:
        return {c: None for c in cams}
    cfg = dict(transform_manager)
    lists = dict(dict(cfg.get("transforms", cfg) or {}).get(split) or {})
    out = {}
    for c in cams:
        kw, seen = {"pad": 0, "prob": 0.0}, False
        for t in lists.get(c) or []:
            t = dict(t)
            name = str(t.get("_target_", "")).rsplit(".", 1)[-1]
            if name == "Resize":
                size = t["size"]
                kw["resize"] = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
            elif name == "RandomShiftsAug":
                kw["pad"], seen = int(t.get("pad", 4)), True
            elif name == "ColorTransform":
                kw.update(brightness=t.get("brightness", 0.0), contrast=t.get("contrast", 0.0), hue=t.get("hue", 0.0),
                          prob=t.get("prob", 1.0))
                seen = True
            elif name == "Normalize":
                if [float(x) for x in t.get("mean", [0.5])] != [0.5] or [float(x) for x in t.get("std", [0.5])] != [0.5]:
                    raise NotImplementedError(f"transform {t.get('_target_')} of {c}: only Normalize(0.5, 0.5) is part of the pack")
            elif name != "ScaleImageTensor":  # (x / 255: part of the pack)
                raise NotImplementedError(f"transform {t.get('_target_')} of {c} is not built")
        out[c] = AugmentSpec(**kw) if seen or "resize" in kw else None
    return out


class RILDataModule:
    """Drop-in for the reference's BasicDataModule with the RILDataset config (config/datamodule/relay_imitation_learning.yaml):
    `Trainer.fit(model, datamodule=dm)`.  `dataset` is the reference's dataset config (max_low_level_window,
    max_high_level_window) plus where the data is: `path`, an .npz with `frames/<camera>` (N,H,W,3) uint8, `actions` (N,A) and
    the episode tables `ep_start_end_ids_train` / `ep_start_end_ids_val` over those N frames, or `arrays`, a dict of the same.
    train_percentage / val_percentage keep the first int(len * p) items (BasicDataModule's Subset); val_percentage 0: no
    validation loader.  `_target_`, `modalities`, `action_type`, `n_digits`, `transf_type`, `num_workers`, `pin_memory`,
    `shuffle_val` are accepted and unused: the dataset is resident and a batch is one kernel launch.
    transform_manager: the `rl` form (see augment_specs); its train list becomes the train loader's augmentation, a Resize
    to the stored size is no stage, and validation batches carry no augmentation - the frames must be stored at the size the
    validation list resizes to.  steps_per_epoch defaults to len(train index) // batch_size; batches are fresh i.i.d. device
    draws with replacement (RelayIndex.draw_device), not the reference's shuffled pass without replacement."""

    def __init__(self, dataset, batch_size=64, train_percentage=1.0, val_percentage=1.0, transform_manager=None,
                 steps_per_epoch=None, val_steps=None, num_workers=4, pin_memory=True, shuffle_val=False, data_dir=None,
                 device=None, fused=True, generator=None, slots=6, **unused):
        bad = [k for k in unused if k not in ("_target_", "_recursive_")]
        if bad:
            raise TypeError(f"RILDataModule: unknown settings {bad}")
        self.dataset_cfg, self.batch_size = dict(dataset), int(batch_size)
        self.train_percentage, self.val_percentage = float(train_percentage), float(val_percentage)
        self.transform_manager, self.steps_per_epoch, self.val_steps = transform_manager, steps_per_epoch, val_steps
        self.device, self.fused, self.generator, self.slots = device, fused, generator, slots
        unknown = [k for k in self.dataset_cfg if k not in _DATASET_KEYS + _DATASET_UNUSED]
        if unknown:
            raise TypeError(f"RILDataModule: unknown dataset settings {unknown}")
        if ("path" in self.dataset_cfg) == ("arrays" in self.dataset_cfg):
            raise ValueError("RILDataModule: give the dataset as `path` (an .npz) or as `arrays`")
        self.cams = self._cameras()
        self.aug_specs = augment_specs(self.transform_manager, self.cams, "train")  # (raises for what is not built)
        self._val_specs = augment_specs(self.transform_manager, self.cams, "validation")
        self.train_replay = self.val_replay = None

    def _cameras(self):
        c = self.dataset_cfg
        if "arrays" in c:
            a = c["arrays"]
            fr = a["frames"] if "frames" in a else {k.split("/", 1)[1]: None for k in a if k.startswith("frames/")}
            return sorted(fr)
        with np.load(c["path"]) as z:
            return sorted(k.split("/", 1)[1] for k in z.files if k.startswith("frames/"))

    def _arrays(self):
        c = self.dataset_cfg
        if "arrays" in c:
            a = c["arrays"]
            frames = a["frames"] if "frames" in a else {k.split("/", 1)[1]: v for k, v in a.items() if k.startswith("frames/")}
            return dict(frames), a["actions"], a["ep_start_end_ids_train"], a.get("ep_start_end_ids_val")
        with np.load(c["path"]) as z:
            missing = [k for k in ("actions", "ep_start_end_ids_train") if k not in z.files]
            if missing or not self.cams:
                raise KeyError(f"{c['path']}: no array named {missing or 'frames/<camera>'}")
            return ({cam: z["frames/" + cam] for cam in self.cams}, z["actions"], z["ep_start_end_ids_train"],
                    z["ep_start_end_ids_val"] if "ep_start_end_ids_val" in z.files else None)

    def prepare_data(self, *args, **kwargs):
        pass

    def setup(self, stage=None):
        if self.train_replay is not None:
            return
        from ..lightning import default_device

        dev = torch.device(self.device if self.device is not None else default_device())  # one process per GPU
        frames, actions, ep_train, ep_val = self._arrays()
        frames = {c: torch.as_tensor(v).to(dev).contiguous() for c, v in frames.items()}  # both splits share the frames
        n = min(int(v.shape[0]) for v in frames.values())
        kw = {k: self.dataset_cfg[k] for k in ("max_low_level_window", "max_high_level_window") if k in self.dataset_cfg}
        for c, v in frames.items():
            stored = tuple(v.shape[1:3])
            sp, vs = self.aug_specs[c], self._val_specs[c]
            if sp is not None and sp.resize == stored:
                sp.resize = None
            resized = [s.resize for s in (sp, vs) if s is not None and s.resize not in (None, stored)]
            if resized and self.val_percentage > 0:
                raise NotImplementedError(f"{c}: validation batches carry no resize - store the frames at {resized[0]}, not {stored}")
        specs = {c: s for c, s in self.aug_specs.items() if s is not None and (s.resize is not None or s.pad or s.prob)}
        self._train_specs = specs or None
        acts = torch.as_tensor(np.asarray(actions, dtype=np.float32)).to(dev)
        ix = RelayIndex(ep_train, n_frames=n, percentage=self.train_percentage, train=True, **kw)
        self.train_replay = HbmRelayReplay(frames, acts, ix, device=dev, batch_size=self.batch_size, slots=self.slots)
        self.index = ix
        if self.val_percentage > 0:
            if ep_val is None:
                raise KeyError("RILDataModule: val_percentage > 0 needs `ep_start_end_ids_val`")
            vix = RelayIndex(ep_val, n_frames=n, percentage=self.val_percentage, train=False, **kw)
            self.val_replay = HbmRelayReplay(frames, acts, vix, device=dev, batch_size=self.batch_size, slots=self.slots)
            if self.val_steps is None:
                self.val_steps = max(len(vix) // self.batch_size, 1)
        if self.steps_per_epoch is None:
            self.steps_per_epoch = len(ix) // self.batch_size
        if int(self.steps_per_epoch) < 1:
            raise ValueError(f"{len(ix)} items give no batch of {self.batch_size}")

    def train_dataloader(self):
        self.setup()
        return RelayLoader(self.train_replay, self.batch_size, self.steps_per_epoch, aug_specs=self._train_specs,
                           generator=self.generator, fused=self.fused)

    def val_dataloader(self):
        self.setup()
        if self.val_replay is None:
            return None
        return RelayLoader(self.val_replay, self.batch_size, self.val_steps, generator=self.generator, train=False,
                           fused=self.fused)
