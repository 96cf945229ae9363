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
from .augment import RIL_ROLES, augment_specs, draw_ril_batch_augmentation  # noqa: F401  (augment_specs: imported from here)
from .resident import (FrameDataModule, ResidentLoader, ResidentReplay, episode_end, index_tables, pick, resident_frames,
                       validate_episodes)

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
        self.ep, self.n_frames = validate_episodes(ep_start_end_ids, n_frames)
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
        """find_episode_end (:115-119): the end of the episode with start <= step <= end."""
        return episode_end(self.ep, step)

    def sample(self, idx, d):
        """idx (n,) items (None: d["idx"]); d = draw(...).  Returns the four frame ids under the SLOTS names, `step`
        (= obs) and `idx`."""
        idx = np.asarray(d["idx"] if idx is None else idx, dtype=np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"item outside [0, {len(self)})")
        u_low, u_high = np.asarray(d["u_low"], dtype=np.float64), np.asarray(d["u_high"], dtype=np.float64)
        step = self.episode_lookup[idx]
        end = self.episode_end(step)
        room = end - step
        sub = np.where(self.low_window >= room, end, step + np.minimum(self.low_window, room))  # min(end, step + Lw)
        hmax = np.where(self.high_window >= room, end, step + np.minimum(self.high_window, room))
        nl, nh = sub - step - 1, hmax - sub
        low = np.where(nl > 0, step + 1 + pick(u_low, np.maximum(nl, 0)), sub)
        high = np.where(nh > 0, sub + pick(u_high, np.maximum(nh, 0)), hmax)
        return {"obs": step, "low_level_goal": low, "high_level_goal": high, "high_level_action": sub, "step": step, "idx": idx}


class HbmRelayReplay(ResidentReplay):
    """RelayImitationLearning's batches out of a dataset resident in HBM (data/resident.py ResidentReplay): frames[cam] =
    (N,H,W,3) uint8, the (N,A) action table and the index tables all live on the device, and `batch()` is one launch of the
    sampler kernel (`tacorl_sample_relay`) on the current stream - no host synchronisation, nothing over PCIe."""

    SUBJECT = "relay replay"
    DRAWS = {"idx": np.int64, "u_low": np.float64, "u_high": np.float64}

    def __init__(self, frames, actions, index, device=None, batch_size=64, slots=6):
        super().__init__(device if device is not None else next(iter(frames.values())).device, index, batch_size, slots)
        self.frames, acts, _ = resident_frames(frames, actions, self.dev, cover=index.n_frames)
        self.tables = {**index_tables(self.dev, index, lookup=index.episode_lookup), "actions": acts, "n_frames": index.n_frames}
        self.A = int(acts.shape[1])
        self._grow(self.batch_size)

    def _slot(self, B):
        return {"ids": (len(SLOTS) * B, torch.int64), "action": (B * self.A, torch.float32)}

    def batch(self, draws=None, aug=None, fused=True, batch_size=None):
        """draws: RelayIndex.draw_device(...) (None: drawn here for `batch_size`), or the host form `draw(...)`.
        fused=True: no frame moves here - the batch carries the dataset tensors and the (4, B) id table in SLOTS order
        (`batch["replay"]`), and RelayImitationLearning's image pack reads the frames by id on their way into the encoder.
        fused=False: the reference dataset's schema - the four role dicts of uint8 (B,H,W,3) frames gathered here
        (tacorl_gather_frames_u8) and `low_level_action`."""
        d = self._draws(draws, batch_size)
        B = int(d["idx"].numel())
        slot, buf = self._next(B)
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


class RelayLoader(ResidentLoader):
    """The loader of RelayImitationLearning (data/resident.py ResidentLoader) over an HbmRelayReplay."""

    def _augment(self, rp):
        return draw_ril_batch_augmentation(self.aug_specs, self.batch_size, rp.dev, self.generator)


class RILDataModule(FrameDataModule):
    """Drop-in for the reference's BasicDataModule with the RILDataset config (config/datamodule/relay_imitation_learning.yaml;
    data/resident.py FrameDataModule says what the two frame datamodules share).  `dataset` is the reference's dataset config
    (max_low_level_window, max_high_level_window) plus `path`, `arrays` or `frame_dir` (the reference's directory; with it
    `modalities`, `action_type` and `n_digits` are read as FrameDataModule says).  `_target_`, `modalities`, `action_type`,
    `n_digits`, `transf_type`, `real_world`, `num_workers`, `pin_memory`, `shuffle_val` are otherwise accepted and unused: the
    dataset is resident and a batch is one kernel launch.  n_frames is what the cameras hold; HbmRelayReplay refuses a shorter action table."""

    DATASET_KEYS = ("max_low_level_window", "max_high_level_window")
    DATASET_UNUSED = ("_target_", "_recursive_", "modalities", "action_type", "n_digits", "transf_type", "real_world")
    LOADER = RelayLoader

    def __init__(self, dataset, batch_size=64, train_percentage=1.0, val_percentage=1.0, transform_manager=None,
                 steps_per_epoch=None, val_steps=None, num_workers=4, pin_memory=True, shuffle_val=False, data_dir=None,
                 device=None, fused=True, generator=None, slots=6, **unused):
        super().__init__(dataset, batch_size, train_percentage, val_percentage, transform_manager, steps_per_epoch, val_steps,
                         device, fused, generator, slots, unused)

    def _index(self, ep, percentage, split, n_frames, dev):
        kw = {k: self.dataset_cfg[k] for k in self.DATASET_KEYS if k in self.dataset_cfg}
        return RelayIndex(ep, n_frames=n_frames, percentage=percentage, train=split == "train", **kw)

    def _replay(self, frames, acts, index, dev):
        return HbmRelayReplay(frames, acts, index, device=dev, batch_size=self.batch_size, slots=self.slots)

