"""The vector-observation (D4RL) data path: the sampling of the reference's D4RLPlayDataset
(datamodule/dataset/d4rl_play_dataset.py:69-146,212-251) as index arithmetic with explicit draws (D4RLWindowIndex), the
dataset resident in HBM with one sampler launch per batch (HbmD4RLReplay, `tacorl_sample_d4rl_windows`), and the loader /
datamodule that `Trainer.fit` takes (D4RLWindowLoader, D4RLDataModule - the counterpart of the reference's
datamodule/d4rl_data_module.py, without gym or d4rl: the four dataset arrays come from an .npz).
The AntMaze dataset is about 1 M frames x 37 floats = 150 MB: it fits in HBM many times over.
"""
import numpy as np
import torch

from .. import ops
from .resident import ResidentLoader, ResidentReplay, episode_end, index_tables, validate_episodes

GOAL_DIM = 2  # the goal is the (x, y) position: observations[goal_step][:2] (:117-118)
NPZ_KEYS = ("observations", "actions", "timeouts", "terminals")  # env.get_dataset()'s names


class D4RLWindowIndex:
    """D4RLPlayDataset.__getitem__ as a deterministic function of explicit draws, as TransitionIndex is for the transitions:
    item idx is the window observations[s : s + ws] / actions[s : s + ws] with s = episode_lookup[idx], padded to
    max_window_size (observations repeat the last row, actions get zero rows); with include_goal the goal is
    observations[min(episode_end, s + (ws - 1) * disp)][:2] and goal_reached = ||goal - observations[s + ws - 1][:2]|| <
    goal_threshold in float32.  tests/golden/d4rl_window_sampler.npz (recorded from the reference class) pins it;
    `tacorl_sample_d4rl_windows` is the same arithmetic on the device.
    Episodes (:212-224): the ends are the sorted union of the set `timeouts` and `terminals`; [start, end] is kept when
    end - start > min_window_size; frames behind the last end belong to no episode.  Items (:241-251): range(start,
    end + 1 - max_window_size) of every kept episode (none for one shorter than max_window_size).
    The tables are validated here, once: every id the arithmetic can then produce lies in [0, n_frames) - the window's rows
    s .. s + max - 1 <= end, the goal step <= end, the reach row s + ws - 1 - which is what the unchecked device reads rely on."""

    def __init__(self, timeouts, terminals, n_frames=None, min_window_size=8, max_window_size=16, pad=True, include_goal=False,
                 goal_sampling_prob=0.3, goal_augmentation=False, goal_threshold=0.5):
        if goal_augmentation:
            raise NotImplementedError("goal_augmentation is set by no config (and turns the reference's goal into float64): not built")
        self.min, self.max = int(min_window_size), int(max_window_size)
        if self.min > self.max:
            raise ValueError(f"min_window_size {self.min} > max_window_size {self.max}")  # :79-84
        if self.min < 2:
            raise NotImplementedError("min_window_size < 2: a one-frame window has no goal displacement (not built)")
        if not pad and self.min != self.max:
            raise NotImplementedError("pad=False with a varying window: the reference cannot collate such a batch")
        if not 0.0 < float(goal_sampling_prob) <= 1.0:
            raise ValueError(f"goal_sampling_prob {goal_sampling_prob} outside (0, 1]")
        self.pad, self.include_goal = bool(pad), bool(include_goal)
        self.p_goal, self.goal_threshold = float(goal_sampling_prob), float(goal_threshold)
        timeouts, terminals = np.asarray(timeouts).reshape(-1), np.asarray(terminals).reshape(-1)
        if len(timeouts) != len(terminals):
            raise ValueError("timeouts and terminals differ in length")
        self.n_frames = int(n_frames) if n_frames is not None else len(timeouts)
        if not 0 < self.n_frames <= len(timeouts):
            raise ValueError(f"n_frames {self.n_frames} outside (0, {len(timeouts)}]")
        ends = np.flatnonzero((timeouts[: self.n_frames] != 0) | (terminals[: self.n_frames] != 0)).astype(np.int64)
        starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64) if len(ends) else ends
        keep = ends - starts > self.min
        self.ep = np.stack([starts[keep], ends[keep]], axis=1).reshape(-1, 2)
        if len(self.ep) == 0:
            raise ValueError("no episode longer than min_window_size + 1")
        if (self.ep[:, 1] <= self.max).any():  # the reference asserts on the absolute index (:246)
            raise ValueError(f"an episode ends at frame {int(self.ep[:, 1].min())} <= max_window_size {self.max}")
        self.episode_lookup = np.concatenate([np.arange(s, max(e + 1 - self.max, s)) for s, e in self.ep]).astype(np.int64)
        if len(self.episode_lookup) == 0:
            raise ValueError("no episode as long as max_window_size: the dataset has no item")
        validate_episodes(self.ep, self.n_frames)
        if (self.episode_lookup + self.max - 1 > self.episode_end(self.episode_lookup)).any():
            raise ValueError("episode tables outside the dataset")

    def __len__(self):
        return len(self.episode_lookup)

    def draw(self, n, rng):
        """The random quantities n items consume: the item, the window size (np.random.randint(min, max + 1), :76-78; the
        constant max when min == max) and the goal's geometric displacement (:135).  int64."""
        win = rng.integers(self.min, self.max + 1, size=n) if self.min < self.max else np.full(n, self.max)
        return {"idx": rng.integers(0, len(self), size=n).astype(np.int64), "window": win.astype(np.int64),
                "disp": rng.geometric(self.p_goal, size=n).astype(np.int64)}

    def draw_device(self, n, device, generator=None):
        """`draw` made by torch on the device (nothing crosses PCIe), items drawn with replacement as
        TransitionIndex.draw_device does.  The reference's DataLoader(shuffle=True) draws WITHOUT replacement: every item
        once per epoch, in a random order.  What is no draw - the window when min == max, the displacement of an index
        without goals (never read) - is one constant tensor per (device, n), shared by the batches and written by nobody."""
        dev, g = torch.device(device), generator
        const = self.__dict__.setdefault("_dev_constants", {})
        if (dev, n) not in const:
            const[dev, n] = (torch.full((n,), self.max, device=dev, dtype=torch.int64), torch.ones(n, device=dev, dtype=torch.int64))
        win, disp = const[dev, n]
        idx = torch.randint(0, len(self), (n,), device=dev, generator=g, dtype=torch.int64)
        if self.min < self.max:
            win = torch.randint(self.min, self.max + 1, (n,), device=dev, generator=g, dtype=torch.int64)
        if self.include_goal:
            disp = torch.empty(n, device=dev, dtype=torch.float64).geometric_(self.p_goal, generator=g).to(torch.int64)
        return {"idx": idx, "window": win, "disp": disp}

    def episode_end(self, step):
        """find_episode_end (:107-111): the end of the episode with start <= step <= end."""
        return episode_end(self.ep, step)

    def sample(self, idx, d, observations, actions):
        """The numpy definition.  idx (n,) items (None: d["idx"]); d = draw(...); observations (N, S), actions (N, A) float32.
        Returns start, window, goal_step, the padded observations (n, max, S) / actions (n, max, A), goal (n, 2) float32 and
        goal_reached (n,) bool (goal and goal_reached also without include_goal: the batch then leaves them out)."""
        idx = np.asarray(d["idx"] if idx is None else idx, dtype=np.int64)
        ws, disp = np.asarray(d["window"], dtype=np.int64), np.asarray(d["disp"], dtype=np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self) or ws.min() < self.min or ws.max() > self.max or disp.min() < 1):
            raise IndexError("draws outside the index (idx in [0, len), window in [min, max], disp >= 1)")
        obs_t, act_t = np.asarray(observations, dtype=np.float32), np.asarray(actions, dtype=np.float32)
        s = self.episode_lookup[idx]
        end = self.episode_end(s)
        t = np.arange(self.max)[None, :]
        rows = s[:, None] + np.minimum(t, ws[:, None] - 1)  # pad_with_repetition: the last row again
        obs = obs_t[rows]
        act = np.where((t < ws[:, None])[..., None], act_t[rows], np.float32(0.0))  # pad_with_zeros
        # min(end, s + (ws - 1) * disp) without the overflow of a huge draw: multiply only where the product stays <= end
        stride = ws - 1
        far = disp > (end - s) // stride
        goal_step = np.where(far, end, s + stride * np.where(far, 0, disp))
        goal = obs_t[goal_step][:, :GOAL_DIM]
        last = obs_t[s + ws - 1][:, :GOAL_DIM]
        dx, dy = goal[:, 0] - last[:, 0], goal[:, 1] - last[:, 1]
        reached = np.sqrt(dx * dx + dy * dy, dtype=np.float32) < np.float32(self.goal_threshold)
        return {"idx": idx, "start": s, "window": ws, "goal_step": goal_step, "observations": obs, "actions": act.astype(np.float32),
                "goal": goal.astype(np.float32), "goal_reached": reached}


class HbmD4RLReplay(ResidentReplay):
    """The D4RL window batches out of a dataset resident in HBM (data/resident.py ResidentReplay): the (N, S) observation and
    (N, A) action tables and the index tables live on the device, and a batch is one launch of the sampler kernel
    (`tacorl_sample_d4rl_windows`) on the current stream - no host synchronisation, nothing over PCIe.  The ring holds the
    dense batches only: a fused batch is its draws, and the module's staging samples into its own buffers (`sample_into`)."""

    SUBJECT = "d4rl replay"
    DRAWS = {"idx": np.int64, "window": np.int64, "disp": np.int64}

    def __init__(self, observations, actions, index, device=None, batch_size=64, slots=6):
        as_t = lambda a: torch.as_tensor(a if torch.is_tensor(a) else np.asarray(a, dtype=np.float32))  # noqa: E731
        obs, acts = as_t(observations), as_t(actions)
        if obs.dim() != 2 or acts.dim() != 2 or obs.shape[0] < index.n_frames or acts.shape[0] < index.n_frames or obs.shape[1] < GOAL_DIM:
            raise ValueError(f"observations (N,S) and actions (N,A) must cover the index's {index.n_frames} frames")
        super().__init__(device if device is not None else obs.device, index, batch_size, slots)
        self.tables = {**index_tables(self.dev, index, lookup=index.episode_lookup),
                       "observations": obs.to(self.dev, torch.float32).contiguous(),
                       "actions": acts.to(self.dev, torch.float32).contiguous(), "n_frames": index.n_frames}
        self.S, self.A, self.T = int(obs.shape[1]), int(acts.shape[1]), index.max
        self.G = GOAL_DIM if index.include_goal else 0
        self._grow(self.batch_size)

    @classmethod
    def from_npz(cls, path, device=None, batch_size=64, slots=6, **index_kwargs):
        """The four arrays by their D4RL key names (`observations`, `actions`, `timeouts`, `terminals`), as
        np.savez(path, **{k: env.get_dataset()[k] for k in ...}) writes them; index_kwargs: D4RLWindowIndex's."""
        with np.load(path) as z:
            missing = [k for k in NPZ_KEYS if k not in z.files]
            if missing:
                raise KeyError(f"{path}: no array named {missing}")
            a = {k: z[k] for k in NPZ_KEYS}
        return cls(a["observations"], a["actions"], D4RLWindowIndex(a["timeouts"], a["terminals"], **index_kwargs),
                   device=device, batch_size=batch_size, slots=slots)

    def _slot(self, B):
        f32, i64 = torch.float32, torch.int64
        return {"obs": (B * self.T * self.S, f32), "act": (B * self.T * self.A, f32), "goal": (B * GOAL_DIM, f32),
                "reached": (B, f32), "window_size": (B, i64), "ids": (2 * B, i64)}

    def sample_into(self, d, obs, actions, goal=None, reached=None, done=None, window_size=None, ids=None):
        """One sampler launch that writes the caller's buffers: obs (B, T, S), actions (B, T, A) and, where given, goal (B, 2),
        reached / done (B) f32 0/1, window_size (B) and ids (2, B) int64 - a training step's own input buffers (fused batch)."""
        if (goal is not None or reached is not None or done is not None) and not self.G:
            raise ValueError("the index was built without include_goal: it has no goal and no goal_reached")
        ops.sample_d4rl_windows(self.tables, d, self.T, self.G, self.index.min, self.index.goal_threshold, obs, actions,
                                self.status, goal=goal, reached=reached, done=done, window_size=window_size, ids=ids)

    def batch(self, draws=None, batch_size=None, fused=False):
        """draws: D4RLWindowIndex.draw_device(...) (None: drawn here for `batch_size`), or the host form `draw(...)`.
        fused=False: the reference dataset's collated batch - `observations` (B, Tmax, S), `actions` (B, Tmax, A) f32, `idx`,
        `window_size` (B) int64 and, with include_goal only, `goal` (B, 2) f32 and `goal_reached` (B) - as views of the ring's
        buffers.  `goal_reached` is the f32 0/1 vector where the reference has a bool: the modules copy_ it into a float
        buffer anyway.
        fused=True: nothing moves here - the batch is {"replay": {"kind": "d4rl_window", "replay": self, "draws", "B", "T"}},
        and the module's staging calls `sample_into` on its own input buffers (tacorl_d4rl.TACORL, play_lmp_d4rl.PlayLMP)."""
        d = self._draws(draws, batch_size)
        B = int(d["idx"].numel())
        if fused:
            return {"replay": {"kind": "d4rl_window", "replay": self, "draws": d, "B": B, "T": self.T}}
        _, buf = self._next(B)
        obs, act = buf["obs"][: B * self.T * self.S].view(B, self.T, self.S), buf["act"][: B * self.T * self.A].view(B, self.T, self.A)
        ws, ids = buf["window_size"][:B], buf["ids"][: 2 * B].view(2, B)
        b = {"observations": obs, "actions": act, "idx": d["idx"], "window_size": ws}
        if self.G:
            b["goal"], b["goal_reached"] = buf["goal"][: B * GOAL_DIM].view(B, GOAL_DIM), buf["reached"][:B]
        self.sample_into(d, obs, act, goal=b.get("goal"), reached=b.get("goal_reached"), window_size=ws, ids=ids)
        return b


class D4RLWindowLoader(ResidentLoader):
    """The loader of the D4RL modules (data/resident.py ResidentLoader) over an HbmD4RLReplay: no augmentation, no validation
    form; a fused batch holds nothing but its draws."""

    def __init__(self, replay, batch_size, steps_per_epoch, generator=None, fused=True):
        super().__init__(replay, batch_size, steps_per_epoch, generator=generator, fused=fused)


_INDEX_KEYS = ("min_window_size", "max_window_size", "pad", "include_goal", "goal_sampling_prob", "goal_augmentation",
               "goal_threshold")


def _vector_transforms(cfg):
    """The (split, modality) pairs of a transform manager config that name a transform for the vector modalities."""
    from collections.abc import Mapping  # (an omegaconf DictConfig is one)

    cfg = dict(cfg or {})
    splits = cfg.get("transforms", cfg)
    return [(s, m) for s, mods in dict(splits or {}).items() if isinstance(mods, Mapping)
            for m in ("observations", "actions") if mods.get(m)]


class D4RLDataModule:
    """Drop-in for the reference's datamodule/d4rl_data_module.py D4RLDataModule: `Trainer.fit(model, datamodule=dm)`.
    `dataset` is the reference's dataset config (config/datamodule/dataset/{d4rl_play_dataset,tacorl_d4rl}.yaml:
    min_window_size, max_window_size, pad, include_goal, goal_sampling_prob, goal_augmentation, goal_threshold) plus where the
    data is: `path`, an .npz of the four arrays of env.get_dataset() (`observations`, `actions`, `timeouts`, `terminals`), or
    `arrays`, a dict of them.  `d4rl_env` (and `_target_`, `transf_type`) are accepted and ignored: nothing here imports gym.
    The `rl` transform manager has no transform for `observations` / `actions`; a config that names one is not built.
    `num_workers` / `pin_memory` are accepted and unused: the dataset is resident and a batch is one kernel launch.
    steps_per_epoch defaults to len(index) // batch_size (draws are with replacement, see D4RLWindowIndex.draw_device)."""

    def __init__(self, dataset, batch_size=32, steps_per_epoch=None, num_workers=4, pin_memory=True, transform_manager=None,
                 device=None, fused=True, generator=None, slots=6):
        self.dataset_cfg, self.batch_size, self.steps_per_epoch = dict(dataset), int(batch_size), steps_per_epoch
        self.num_workers, self.pin_memory, self.device, self.fused = num_workers, pin_memory, device, fused
        self.generator, self.slots = generator, slots
        named = _vector_transforms(transform_manager)
        if named:
            raise NotImplementedError(f"transforms for vector modalities are not built: {named}")
        unknown = [k for k in self.dataset_cfg if k not in _INDEX_KEYS + ("path", "arrays", "d4rl_env", "_target_", "_recursive_",
                                                                          "transf_type", "transform_manager")]
        if unknown:
            raise TypeError(f"D4RLDataModule: unknown dataset settings {unknown}")
        if ("path" in self.dataset_cfg) == ("arrays" in self.dataset_cfg):
            raise ValueError("D4RLDataModule: give the dataset as `path` (an .npz) or as `arrays`")
        self.replay = None

    def prepare_data(self, *args, **kwargs):
        pass

    def setup(self, stage=None):
        if self.replay is not None:
            return
        c = self.dataset_cfg
        kw = {k: c[k] for k in _INDEX_KEYS if k in c}
        from ..lightning import default_device

        dev = self.device if self.device is not None else default_device()  # one process per GPU: each rank its own replay
        if "path" in c:
            self.replay = HbmD4RLReplay.from_npz(c["path"], device=dev, batch_size=self.batch_size, slots=self.slots, **kw)
        else:
            a = c["arrays"]
            self.replay = HbmD4RLReplay(a["observations"], a["actions"], D4RLWindowIndex(a["timeouts"], a["terminals"], **kw),
                                        device=dev, batch_size=self.batch_size, slots=self.slots)
        self.index = self.replay.index
        if self.steps_per_epoch is None:
            self.steps_per_epoch = len(self.index) // self.batch_size
        if int(self.steps_per_epoch) < 1:
            raise ValueError(f"{len(self.index)} items give no batch of {self.batch_size}")

    def train_dataloader(self):
        self.setup()
        return D4RLWindowLoader(self.replay, self.batch_size, self.steps_per_epoch, generator=self.generator, fused=self.fused)
