"""The play-window data path on the device (`experiment=tacorl`, `play_lmp_for_rl` and the real-world variants): the dataset
resident in HBM with one sampler launch per batch (HbmPlayReplay, `tacorl_sample_play_windows` - PlayIndex.sample and
pad_actions of data/replay.py as index arithmetic over resident tables), and the loader / datamodule that `Trainer.fit`
takes (PlayWindowLoader, PlayDataModule - the counterpart of the reference's datamodule/basic_data_module.py BasicDataModule
with the PlayDataset configs).  Beside data/replay.py's HbmReplay / prefetching, which sample on the host and stage every
batch through pinned memory on a feeder thread: here the trainer's own thread enqueues the draws and the sampler in front of
the step, and nothing is synchronised, copied or allocated per batch.
"""
import os

import numpy as np
import torch

from .. import ops
from .augment import draw_play_batch_augmentation
from .replay import PlayIndex
from .resident import (FrameDataModule, ResidentLoader, ResidentReplay, index_tables, is_table, neighbour_tables,
                       resident_frames, validate_episodes)


def validate_play_tables(index, n_frames):
    """The tables of a PlayIndex against a dataset of n_frames frames, once: the episode bounds lie inside [0, n_frames), the
    episodes are sorted by start and do not overlap, every item leaves room for a max-size window inside its episode
    (episode_lookup[i] + max_ws - 1 <= the end of the episode that holds it), and every neighbour key and value lies inside
    [0, n_frames).  Every id the sampler's arithmetic can then produce is a frame of the dataset - the window
    s .. s + ws - 1 <= end, a geometric goal <= end (clipped at 0), a neighbour checked one by one, a random state another
    item - which is what the unchecked device gathers behind it rely on."""
    n_frames = int(n_frames)
    ep = np.asarray(index.ep, dtype=np.int64).reshape(-1, 2)
    if len(ep) == 0:
        raise ValueError("play replay: no episodes")
    if index.min_ws < 1:
        raise ValueError(f"play replay: min_window_size {index.min_ws} < 1")
    if n_frames < index.max_ws:
        raise ValueError(f"play replay: {n_frames} frames hold no window of {index.max_ws}")
    validate_episodes(ep, n_frames, what="play replay: ")
    look = np.asarray(index.episode_lookup, dtype=np.int64)
    if len(look) == 0:
        raise ValueError("play replay: the index has no item")
    end = index.episode_end(look)  # -1 where an item lies in no episode
    if (look < 0).any() or (look + index.max_ws - 1 > end).any():
        raise ValueError("play replay: an item's max-size window leaves its episode")
    ptr, val = np.asarray(index._nn_ptr, dtype=np.int64), np.asarray(index._nn_val, dtype=np.int64)
    keys = index.nn_table.host()[2] if index.nn_table is not None else np.array(sorted(index.nn or {}), dtype=np.int64)
    if (len(keys) and (keys.min() < 0 or keys.max() >= n_frames)) or len(ptr) - 1 > n_frames:
        raise ValueError(f"play replay: nn_steps_from_step has a key outside [0, {n_frames})")
    if len(val) and (val.min() < 0 or val.max() >= n_frames):
        raise ValueError(f"play replay: nn_steps_from_step has a neighbour outside [0, {n_frames})")
    if len(ptr) < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] > len(val):
        raise ValueError("play replay: the neighbour CSR is not a row pointer over its values")


class HbmPlayReplay(ResidentReplay):
    """The play-window batches out of a dataset resident in HBM (data/resident.py ResidentReplay): frames[cam] = (N,H,W,3)
    uint8, the (N,A) action table and the index tables (episode_lookup, the episode bounds, the neighbour CSR) all live on the
    device, and `batch()` is one launch of the sampler kernel (`tacorl_sample_play_windows`) on the current stream - no host
    synchronisation, nothing over PCIe, no feeder thread.  The tables are validated here, once (validate_play_tables); the
    dataset is as long as its shortest table.
    include_goal=False (PlayLMP's dataset, config/datamodule/dataset/play_dataset.yaml): the batch carries no `goal` and no
    `disp`, as the reference's."""

    SUBJECT = "play replay"
    DRAWS = {"idx": np.int64, "window_size": np.int64, "strategy": np.int64, "disp": np.int64, "noise_step": np.int64,
             "u_choice": np.float64, "u_random_state": np.float64}

    def __init__(self, frames, actions, index, device=None, batch_size=64, slots=6, include_goal=True):
        dev = torch.device(device if device is not None else torch.as_tensor(next(iter(frames.values()), actions)).device)
        self.frames, acts, n_frames = resident_frames(frames, actions, dev)
        validate_play_tables(index, n_frames)
        super().__init__(dev, index, batch_size, slots)
        self.include_goal = bool(include_goal)
        self.tables = {**index_tables(dev, index, lookup=index.episode_lookup), **neighbour_tables(index, dev), "actions": acts,
                       "n_frames": n_frames, "last_end": int(index.ep[:, 1].max())}
        self.A, self.T = int(acts.shape[1]), index.max_ws
        self._grow(self.batch_size)

    def _slot(self, B):
        return {"ids": (B * self.T + B, torch.int64), "act": (B * self.T * self.A, torch.float32), "disp": (B, torch.int64),
                "window_size": (B, torch.int64)}

    def _draws(self, draws, batch_size=None):
        d = super()._draws(draws, batch_size)
        if self.index.min_ws == self.index.max_ws:  # the window is no draw (PlayIndex.sample ignores it too)
            d["window_size"] = self.index.device_constants(int(d["idx"].numel()), self.dev)[0]
        return d

    def batch(self, draws=None, aug=None, fused=True, batch_size=None):
        """draws: PlayIndex.draw_device(...) (None: drawn here for `batch_size`), or the host form `draw(...)` with `idx`.
        The schema is HbmReplay.batch's without `ready` (there is no copy stream to wait for):
        fused=True: no frame moves here - the batch carries the dataset tensors and the id table [B*T window frames | B goal
        frames] (`batch["replay"]`), and the module's image pack reads the frames by id on their way into the encoder.
        fused=False: `states` (B,T,H,W,3) / `goal` (B,H,W,3) uint8 per camera, gathered here (tacorl_gather_frames_u8).
        Both: `actions` (B,T,A) f32, `disp`, `idx`, `window_size` (B) int64 on the device, and `aug` where given."""
        d = self._draws(draws, batch_size)
        B, T = int(d["idx"].numel()), self.T
        slot, buf = self._next(B)
        ids, act = buf["ids"][: B * T + B], buf["act"][: B * T * self.A].view(B, T, self.A)
        disp, ws = buf["disp"][:B], buf["window_size"][:B]
        ops.sample_play_windows(self.tables, d, T, self.index.min_ws, ids, act, disp, ws, self.status,
                                goal_augmentation=self.index.goal_augmentation)
        b = {"actions": act, "idx": d["idx"], "window_size": ws}
        if self.include_goal:
            b["disp"] = disp
        if aug is not None:
            b["aug"] = aug
        if fused:
            b["replay"] = {"frames": self.frames, "ids": ids, "B": B, "T": T}
            return b
        states, goal = {}, {}
        for c, fr in self.frames.items():
            H, W = fr.shape[1:3]
            states[c] = ops.gather_frames_u8(fr, ids[: B * T], self._out((slot, "s", c), (B, T, H, W, 3)))
            if self.include_goal:
                goal[c] = ops.gather_frames_u8(fr, ids[B * T:], self._out((slot, "g", c), (B, H, W, 3)))
        b["states"] = states
        if self.include_goal:
            b["goal"] = goal
        return b


class PlayWindowLoader(ResidentLoader):
    """The loader of TACORL and PlayLMP (data/resident.py ResidentLoader) over an HbmPlayReplay: a training batch carries
    draw_play_batch_augmentation(aug_specs, ...), one draw per frame of the window and one for the goal frame."""

    def _augment(self, rp):
        return draw_play_batch_augmentation(self.aug_specs, self.batch_size, rp.T, rp.dev, self.generator)


_INDEX_KEYS = ("min_window_size", "max_window_size", "goal_sampling_prob", "goal_strategy_prob", "goal_augmentation")


class PlayDataModule(FrameDataModule):
    """Drop-in for the reference's BasicDataModule with the PlayDataset configs (config/datamodule/{tacorl,play_lmp}.yaml with
    dataset/{tacorl,play_dataset}.yaml; data/resident.py FrameDataModule says what the two frame datamodules share).  `dataset`
    is the reference's dataset config (min_window_size, max_window_size, pad, include_goal, goal_sampling_prob,
    goal_strategy_prob, goal_augmentation) plus `path`, `arrays` or `frame_dir`; n_frames is what the cameras and the action
    table hold.  With `frame_dir` (the reference's directory; FrameDataModule says how) `action_type`, `n_digits`,
    `num_nn` and the cameras of `modalities` are read (`real_world` stays without effect), and a neighbour table that is needed
    comes from the reference's step-keyed JSON - the path given as nn_steps_from_step, the config's nn_steps_from_step_path,
    nn_steps_from_step.json beside training/ or in the split's directory - remapped to rows, or is built from robot_obs and
    written there; a NeighbourTable or dict given outright is in rows of the compacted arrays.
    include_goal false (PlayLMP's play_dataset.yaml): the batch has no `goal` and no `disp`, and no neighbour table is read.
    `nn_steps_from_step` (here or in `dataset`; `nn_steps_from_step_val` for the validation split): a NeighbourTable
    (data/neighbours.py), the reference's dict {step: [steps]}, or the path of the reference's JSON file, read with
    NeighbourTable.load_json ("train" / "validation"); the config's `nn_steps_from_step_path` is read the same way where it
    names an existing file and no table was given.  Without a table a similar_robot_obs goal is the reference's fallback, a
    random state.  pad must be true: the reference cannot collate unpadded windows of varying length either.  `_target_`,
    `modalities`, `action_type`, `n_digits`, `transf_type`, `num_nn`, `real_world`, `num_workers`, `pin_memory`, `shuffle_val`,
    `data_dir` are accepted and unused (without `frame_dir`: all of them): the dataset is resident and a batch is one kernel
    launch.  Validation batches are device draws like the training ones (as RILDataModule's): the reference chooses a validation
    window size with hash(str(idx)), which Python salts per process, so its validation set is not reproducible from run to
    run even there."""

    DATASET_KEYS = _INDEX_KEYS + ("pad", "include_goal", "nn_steps_from_step", "nn_steps_from_step_val", "nn_steps_from_step_path")
    DATASET_UNUSED = ("_target_", "_recursive_", "modalities", "action_type", "n_digits", "transf_type", "transform_manager",
                      "num_nn", "real_world", "skip_frames", "data_dir", "train")
    LOADER = PlayWindowLoader

    def __init__(self, dataset, batch_size=64, train_percentage=1.0, val_percentage=1.0, transform_manager=None,
                 steps_per_epoch=None, val_steps=None, num_workers=4, pin_memory=True, shuffle_val=False, data_dir=None,
                 create_vis_dataset=False, nn_steps_from_step=None, nn_steps_from_step_val=None, device=None, fused=True,
                 generator=None, slots=6, **unused):
        if create_vis_dataset:
            raise NotImplementedError("PlayDataModule: create_vis_dataset is not built")
        if not dict(dataset).get("pad", True):
            raise NotImplementedError("PlayDataModule: pad=false (windows of varying length cannot be collated)")
        for p, name in ((train_percentage, "train_percentage"), (val_percentage, "val_percentage")):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"PlayDataModule: {name} {p} outside [0, 1]")
        super().__init__(dataset, batch_size, train_percentage, val_percentage, transform_manager, steps_per_epoch, val_steps,
                         device, fused, generator, slots, unused)
        c = self.dataset_cfg
        self.include_goal = bool(c.get("include_goal", False))
        self.index_kwargs = {k: c[k] for k in _INDEX_KEYS if k in c}
        if "goal_strategy_prob" in self.index_kwargs:
            self.index_kwargs["goal_strategy_prob"] = dict(self.index_kwargs["goal_strategy_prob"])
        self._nn = {"train": nn_steps_from_step if nn_steps_from_step is not None else c.get("nn_steps_from_step"),
                    "validation": nn_steps_from_step_val if nn_steps_from_step_val is not None else c.get("nn_steps_from_step_val")}

    def _n_frames(self, frames, acts):
        return min([int(v.shape[0]) for v in frames.values()] + [int(acts.shape[0])])

    def _wants_table(self):
        """include_goal with a similar_robot_obs share (the reference's default strategy gives it one half)."""
        gs = self.index_kwargs.get("goal_strategy_prob")
        return self.include_goal and (gs is None or float(gs.get("similar_robot_obs", 0.0)) > 0.0)

    def _nn_file(self, split):
        """With `frame_dir`: (the file that holds - or will receive - the split's step-keyed table, whether it holds it), or
        None where a table was given outright (a NeighbourTable or dict: those are in ROWS of the compacted arrays) or none
        is wanted.  A path given as nn_steps_from_step(_val) and the config's nn_steps_from_step_path go first
        (frame_dir.neighbour_file); the reference's JSON is keyed by step number and is remapped to rows when it is read."""
        if not self._wants_table():
            return None
        nn = self._nn[split]
        if nn is None and split == "validation" and isinstance(self._nn["train"], (str, os.PathLike)):
            nn = self._nn["train"]  # the reference's file holds both splits
        if nn is not None and not isinstance(nn, (str, os.PathLike)):
            return None
        from .frame_dir import neighbour_file

        c = self.dataset_cfg
        return neighbour_file(c["frame_dir"], self._dirs[split], split, (nn, c.get("nn_steps_from_step_path")))

    def _want_robot_obs(self, split):
        """With `frame_dir`: robot_obs is loaded where the split's neighbour table has to be built - none was given and no
        file holds the split's."""
        f = self._nn_file(split)
        return f is not None and not f[1]

    def _neighbours(self, split, n_frames, dev):
        """The split's nn_steps_from_step as PlayIndex takes it (a NeighbourTable or a dict), or None.  With `frame_dir`: the
        step-keyed file _nn_file finds, or the table built from robot_obs and written there (frame_dir.split_neighbours),
        remapped to rows; `num_nn` is then read.  A NeighbourTable or dict given outright is taken in rows, as without
        `frame_dir`."""
        if not self.include_goal:
            return None
        from .neighbours import NeighbourTable

        nn = self._nn[split]
        if "frame_dir" in self.dataset_cfg:
            f = self._nn_file(split)
            if f is not None:
                from .frame_dir import split_neighbours

                return split_neighbours(self.splits[split], dev, num_nn=int(self.dataset_cfg.get("num_nn", 32)), path=f[0])
            if isinstance(nn, (str, os.PathLike)):
                nn = None  # (no similar_robot_obs share: the file is not read)
        if nn is None:
            path = self.dataset_cfg.get("nn_steps_from_step_path")
            nn = path if path and os.path.isfile(os.path.expanduser(str(path))) else None
            if nn is None and split == "validation" and isinstance(self._nn["train"], (str, os.PathLike)):
                nn = self._nn["train"]  # the reference's file holds both splits
        if isinstance(nn, (str, os.PathLike)):
            try:
                return NeighbourTable.load_json(nn, split, n_frames, device=dev)
            except KeyError:
                if split == "train":
                    raise
                return None
        return nn.to(dev) if is_table(nn) else nn

    def _index(self, ep, percentage, split, n_frames, dev):
        ix = PlayIndex(ep, nn_steps_from_step=self._neighbours(split, n_frames, dev), train=split == "train", **self.index_kwargs)
        ix.episode_lookup = ix.episode_lookup[: int(len(ix.episode_lookup) * percentage)]  # BasicDataModule's Subset
        if len(ix) == 0:
            raise ValueError(f"PlayDataModule: the {split} index has no item (percentage {percentage})")
        return ix

    def _replay(self, frames, acts, index, dev):
        return HbmPlayReplay(frames, acts, index, device=dev, batch_size=self.batch_size, slots=self.slots,
                             include_goal=self.include_goal)

