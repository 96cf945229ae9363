"""What the resident data paths share (data/replay.py HbmTransitionReplay, d4rl_replay.py, relay_replay.py, play_replay.py).
A resident replay keeps the whole dataset and its index tables in HBM; a batch is fresh device draws and ONE launch of a sampler
kernel on the current stream - no host synchronisation, nothing over PCIe, no feeder thread - and its tensors are views of the
replay's own ring of `slots` buffer sets.  Here, once:

* the index helpers (`episode_end`, `validate_episodes`, `neighbour_csr`, `pick`) of the four index classes;
* `ResidentReplay`, the base of the four replays: the ring, the status word, the draw normaliser;
* `ResidentLoader`, the loader `Trainer.fit` takes, and `FrameDataModule`, the datamodule of the uint8 frame datasets.
"""
import os

import numpy as np
import torch

from .. import ops
from .augment import augment_specs


# ------------------------------------------------------------------------------------------------------- index helpers
def episode_end(ep, step, missing=None):
    """The reference's find_episode_end by binary search over the sorted starts of ep (E, 2): the end (inclusive) of the last
    episode whose start is <= step.  missing=None: as it stands (episode 0 for a step before the first start) - the tables
    of such an index hold no step outside an episode.  Otherwise `missing` where no episode holds the step."""
    step = np.asarray(step)
    k = np.maximum(np.searchsorted(ep[:, 0], step, side="right") - 1, 0)
    end = ep[k, 1]
    return end if missing is None else np.where((ep[k, 0] <= step) & (step <= end), end, missing)


def validate_episodes(ep, n_frames=None, what=""):
    """ep_start_end_ids as the int64 (E, 2) table, and n_frames (None: the last end + 1).  Refuses (ValueError) an empty
    table, bounds outside [0, n_frames), an end before its start, and episodes that are not sorted by start or overlap."""
    ep = np.asarray(ep, dtype=np.int64).reshape(-1, 2)
    if len(ep) == 0:
        raise ValueError(f"{what}no episodes")
    n_frames = int(n_frames) if n_frames is not None else int(ep[:, 1].max()) + 1
    if ep.min() < 0 or ep.max() >= n_frames:
        raise ValueError(f"{what}episode bounds outside [0, {n_frames})")
    if (ep[:, 0] > ep[:, 1]).any() or (ep[1:, 0] <= ep[:-1, 1]).any():
        raise ValueError(f"{what}episodes must be sorted by start and must not overlap")
    return ep, n_frames


def is_table(nn_steps_from_step):
    """A neighbours.NeighbourTable (the CSR itself) rather than the reference's dict {step: [steps]}."""
    return hasattr(nn_steps_from_step, "index_csr")


def neighbour_csr(nn_steps_from_step, n_frames=None):
    """nn_steps_from_step as (nn_table, nn, ptr, val): the ragged neighbour lists as one int64 CSR indexed by frame id (rows
    [0, max key]).  A NeighbourTable (data/neighbours.py) is that CSR already - adopted as it stands, no loop over its keys,
    nn = None; a dict (or None) becomes {int: int64 array}, nn_table = None.  With n_frames every key and every neighbour
    must lie in [0, n_frames) - a dict is checked key by key, before its CSR is built."""
    if is_table(nn_steps_from_step):
        tab = nn_steps_from_step
        ptr, val = tab.index_csr()
        keys = tab.host()[2]
        if n_frames is not None and ((len(keys) and (keys.min() < 0 or keys.max() >= n_frames))
                                     or (len(val) and (val.min() < 0 or val.max() >= n_frames))):
            raise ValueError(f"nn_steps_from_step: a step outside [0, {n_frames})")
        return tab, None, ptr, val
    nn = {int(k): np.asarray(v, dtype=np.int64).reshape(-1) for k, v in (nn_steps_from_step or {}).items()}
    if n_frames is not None:
        for k, v in nn.items():
            if not 0 <= k < n_frames or (len(v) and (v.min() < 0 or v.max() >= n_frames)):
                raise ValueError(f"nn_steps_from_step[{k}]: a step outside [0, {n_frames})")
    cnt = np.zeros((max(nn) + 1) if nn else 0, dtype=np.int64)
    for k, v in nn.items():
        cnt[k] = len(v)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return None, nn, ptr, np.concatenate([nn[k] for k in sorted(nn)] + [np.zeros(0, np.int64)]).astype(np.int64)


def pick(u, n):
    """floor(u * n) kept inside [0, n): the choice np.random.choice makes among n options, as a function of its uniform."""
    return np.clip((u * n).astype(np.int64), 0, np.maximum(n - 1, 0))


# ------------------------------------------------------------------------------------------------------ resident tables
def i64_table(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def index_tables(dev, index, **items):
    """The int64 device tables every sampler reads: the index's item table under its name, `ep_start` and `ep_end`."""
    return {k: i64_table(a, dev) for k, a in {**items, "ep_start": index.ep[:, 0], "ep_end": index.ep[:, 1]}.items()}


def resident_frames(frames, actions, dev, cover=None):
    """frames {camera: uint8 (N,H,W,3)} and the (N,A) action table on the device (what is there already stays where it is),
    and the number of frames both hold.  cover: the frames an index needs - fewer are refused."""
    acts = torch.as_tensor(np.asarray(actions, dtype=np.float32) if not torch.is_tensor(actions) else actions)
    frames = {c: torch.as_tensor(v) for c, v in frames.items()}
    bad = [c for c, v in frames.items() if v.dtype != torch.uint8 or v.dim() != 4]
    if bad or acts.dim() != 2:
        raise ValueError(f"frames must be uint8 (N,H,W,3) and actions (N,A): {bad or tuple(acts.shape)}")
    n = min([int(v.shape[0]) for v in frames.values()] + [int(acts.shape[0])])
    if cover is not None and n < cover:
        raise ValueError(f"frames (uint8 (N,H,W,3)) and actions (N,A) must cover the index's {cover} frames")
    return {c: v.to(dev).contiguous() for c, v in frames.items()}, acts.to(dev, torch.float32).contiguous(), n


def neighbour_tables(index, dev):
    """The index's neighbour CSR as the sampler's `nn_ptr`, `nn_val` and `n_nn`.  A NeighbourTable built on this device is
    adopted: its tensors are the tables (ptr cut as the index keeps it).  An empty value table gets a one-element stand-in."""
    tab = getattr(index, "nn_table", None)
    if tab is not None and tab.val.numel() and tab.device == torch.empty(0, device=dev).device:
        ptr, val = tab.ptr[: len(index._nn_ptr)], tab.val
    else:
        ptr, val = i64_table(index._nn_ptr, dev), i64_table(index._nn_val if len(index._nn_val) else [0], dev)
    return {"nn_ptr": ptr, "nn_val": val, "n_nn": len(index._nn_ptr) - 1}


# -------------------------------------------------------------------------------------------------------------- replay
class ResidentReplay:
    """The base of the resident replays.  A subclass builds `tables`, states what one ring slot of capacity B holds
    (`_slot(B)`: {name: (elements, dtype)}), the draws its sampler reads (`DRAWS`: {key: host dtype}) and `batch()`.
    The returned tensors are views of this object's own buffers, a ring of `slots` sets: a batch stays valid until
    `slots - 1` more have been drawn, so a trainer that fetches a batch or two ahead of the step it runs (pytorch_lightning
    looks one ahead to learn which batch is the last) still trains on the batch it was given."""

    SUBJECT = "resident replay"
    DRAWS = {}

    def __init__(self, device, index, batch_size, slots):
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        self.dev, self.index, self.batch_size = torch.device(device), index, int(batch_size)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._cap, self._ring, self._k, self._u8 = 0, [{} for _ in range(int(slots))], 0, {}

    def _grow(self, B):
        """The batch buffers exist before the first batch and are replaced only for a larger one - under the capture lock (a
        hipMalloc beside a hipGraph capture on another thread can invalidate it), and captured graphs that could hold an old
        address are dropped (ops.note_alloc)."""
        if B <= self._cap:
            return
        with ops.capture_lock:
            for k in range(len(self._ring)):
                self._ring[k] = {name: torch.zeros(n, dtype=dt, device=self.dev) for name, (n, dt) in self._slot(B).items()}
            self._cap = B
            ops.note_alloc()

    def _next(self, B):
        """(slot, its buffers) for a batch of B: the ring's next set, grown first where B exceeds the capacity."""
        self._grow(B)
        self._k = slot = (self._k + 1) % len(self._ring)
        return slot, self._ring[slot]

    def _out(self, key, shape):
        """The uint8 buffer of a dense batch's gathered frames, kept per key (the slot is part of it)."""
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
            raise IndexError(f"{self.SUBJECT}: the sampler had to clamp a value (tables or draws outside the dataset)")

    def _draws(self, draws, batch_size=None):
        """draws: the index's draw_device(...) (None: drawn here for `batch_size`), or the host form draw(...) - a pageable
        copy: tests and tools, not the training path.  Returns the sampler's keys as contiguous tensors on the device."""
        if draws is None:
            return self.index.draw_device(batch_size or self.batch_size, self.dev)
        d = {}
        for k, dt in self.DRAWS.items():
            if k not in draws:
                raise KeyError(f"{self.SUBJECT}: the draws have no `{k}` (the index's draw_device, or draw() with `idx`)")
            v = draws[k]
            d[k] = (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=dt))).to(self.dev).contiguous()
        return d


# -------------------------------------------------------------------------------------------------------------- loader
class ResidentLoader:
    """`steps_per_epoch` batches of `batch_size` fresh device draws per pass: what Trainer.fit takes as train_dataloaders /
    val_dataloaders.  A training batch carries the subclass's augmentation draw (`_augment`) where aug_specs is given;
    train=False (validation) draws none.  A batch is views of the replay's ring of buffers (slots=6): a trainer may hold up
    to `slots - 1` batches ahead of the one it is running."""

    def __init__(self, replay, batch_size, steps_per_epoch, aug_specs=None, generator=None, train=True, fused=True):
        self.replay, self.batch_size, self.steps_per_epoch = replay, int(batch_size), int(steps_per_epoch)
        self.aug_specs, self.generator, self.train, self.fused = aug_specs, generator, train, fused

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        rp = self.replay
        for _ in range(self.steps_per_epoch):
            draws = rp.index.draw_device(self.batch_size, rp.dev, self.generator)
            aug = {"aug": self._augment(rp)} if self.train and self.aug_specs else {}
            yield rp.batch(draws, fused=self.fused, **aug)


# ---------------------------------------------------------------------------------------------------------- datamodule
class FrameDataModule:
    """The base of the datamodules over uint8 frame datasets (RILDataModule, PlayDataModule), drop-ins for the reference's
    BasicDataModule: `Trainer.fit(model, datamodule=dm)`.  `dataset` is the reference's dataset config plus where the data
    is: `path`, an .npz with `frames/<camera>` (N,H,W,3) uint8, `actions` (N,A) and the episode tables
    `ep_start_end_ids_train` / `ep_start_end_ids_val` over those N frames, or `arrays`, a dict of the same, or `frame_dir`,
    the reference's dataset directory (data/frame_dir.py): a root holding training/ and validation/ - what BasicDataModule
    appends to data_dir, so the yaml line is `frame_dir: ${data_dir}`; each split then has its own frame arrays - or a single
    split directory whose split.json supplies both tables over one shared array.  With `frame_dir` the reference's
    `modalities` (its rgb_* entries are the cameras; absent: the first frame's rgb_* arrays), `action_type` and `n_digits`
    are read; otherwise they stay accepted and unused.  `real_world` stays without effect either way: in the reference it
    only drops scene_obs and state_info, which a replay never holds.  `workers` (8, at most 16), `chunk_frames` (256) and
    `ring` (3) size the loader; `cache_dir` keeps the compacted arrays as .npy for later starts; beside `path` or
    `arrays` these keys are refused.  A missing file, a missing key and a frame whose shape differs from the first frame's
    are refused with the file name before anything is uploaded (every file's array headers are read first).  Under world_size > 1
    every rank loads the same directory: frames are not sharded.
    `store_size: [H, W]` (or {camera: [H, W]}; with `frame_dir` only; default none): every uploaded chunk passes
    tacorl_resize_frames_u8 and the replay holds (N,H,W,3).  With store_size equal to what the train and validation lists
    resize to, the Resize stage is no stage and validation loaders exist.  The one deviation: a batch is then the
    reference's pipeline applied to frames that were resized and ROUNDED TO uint8 when they were stored (at most half a
    grey level per value), not a resize of the float frame at sample time.  Without store_size nothing changes.
    train_percentage / val_percentage keep the first int(len * p) items (BasicDataModule's Subset); val_percentage 0: no
    validation loader.  transform_manager: the `rl` form (see augment.augment_specs); its train list becomes the train
    loader's augmentation, a Resize to the stored size is no stage, and validation batches carry no augmentation - the frames
    must be stored at the size the validation list resizes to.  steps_per_epoch defaults to len(train index) // batch_size,
    val_steps to len(validation index) // batch_size (at least 1); batches are fresh i.i.d. device draws with replacement,
    not the reference's shuffled pass without replacement.
    A subclass states DATASET_KEYS (with DATASET_UNUSED: accepted and unused), LOADER, `_index` and `_replay`."""

    DATASET_KEYS = DATASET_UNUSED = ()
    LOADER = ResidentLoader
    SOURCES = ("path", "arrays", "frame_dir")
    FRAME_DIR_KEYS = ("store_size", "cache_dir", "workers", "chunk_frames", "ring")

    def __init__(self, dataset, batch_size, train_percentage, val_percentage, transform_manager, steps_per_epoch, val_steps,
                 device, fused, generator, slots, unused):
        name = type(self).__name__
        bad = [k for k in unused if k not in ("_target_", "_recursive_")]
        if bad:
            raise TypeError(f"{name}: unknown settings {bad}")
        self.dataset_cfg, self.batch_size = dict(dataset), int(batch_size)
        self.train_percentage, self.val_percentage = float(train_percentage), float(val_percentage)
        self.transform_manager, self.steps_per_epoch, self.val_steps = transform_manager, steps_per_epoch, val_steps
        self.device, self.fused, self.generator, self.slots = device, fused, generator, slots
        unknown = [k for k in self.dataset_cfg if k not in self.DATASET_KEYS + self.DATASET_UNUSED + self.SOURCES + self.FRAME_DIR_KEYS]
        if unknown:
            raise TypeError(f"{name}: unknown dataset settings {unknown}")
        if "frame_dir" in self.dataset_cfg:
            if "path" in self.dataset_cfg or "arrays" in self.dataset_cfg:
                raise ValueError(f"{name}: give exactly one of `path`, `arrays` and `frame_dir`")
        elif ("path" in self.dataset_cfg) == ("arrays" in self.dataset_cfg):
            raise ValueError(f"{name}: give the dataset as `path` (an .npz) or as `arrays`")
        stray = [k for k in self.FRAME_DIR_KEYS if k in self.dataset_cfg and "frame_dir" not in self.dataset_cfg]
        if stray:
            raise ValueError(f"{name}: {stray} belong to the `frame_dir` source (store_size resizes its frames as they are uploaded)")
        self.load_stats = {}
        self.cams = self._cameras()
        self.aug_specs = augment_specs(self.transform_manager, self.cams, "train")  # (raises for what is not built)
        self._val_specs = augment_specs(self.transform_manager, self.cams, "validation")
        self.train_replay = self.val_replay = None

    def _cameras(self):
        c = self.dataset_cfg
        if "frame_dir" in c:
            from .frame_dir import split_dirs

            self._dirs, self._one_dir = split_dirs(c["frame_dir"])
            cams = sorted(m for m in (c.get("modalities") or ()) if str(m).startswith("rgb_"))
            if not cams:
                first = min(e.name for e in os.scandir(self._dirs["train"]) if e.name.endswith(".npz"))
                with np.load(os.path.join(self._dirs["train"], first)) as z:
                    cams = sorted(k for k in z.files if k.startswith("rgb_"))
            if not cams:
                raise KeyError(f"{c['frame_dir']}: no rgb_* camera in `modalities` or in the first frame")
            return cams
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

    def _n_frames(self, frames, acts):
        """The frames the index tables may name: what every camera holds."""
        return min(int(v.shape[0]) for v in frames.values())

    def _settle_resize(self, stored):
        """stored {camera: (H, W)}: a train Resize to the stored size is no stage; a list that resizes away from it is
        refused where a validation loader is asked for.  (With `frame_dir` this runs on the planned sizes, before the load.)"""
        for c, hw in stored.items():
            sp, vs = self.aug_specs[c], self._val_specs[c]
            if sp is not None and sp.resize == hw:
                sp.resize = None
            resized = [s.resize for s in (sp, vs) if s is not None and s.resize not in (None, hw)]
            if resized and self.val_percentage > 0:
                raise NotImplementedError(f"{c}: validation batches carry no resize - store the frames at {resized[0]}, not {hw}")

    def _frame_dir_splits(self, dev):
        """The `frame_dir` source: (frames, actions, ep) in rows for the train split and (or None) for the validation split;
        self.splits keeps each split's frame_dir.LoadedSplit (its compaction, its robot_obs where _want_robot_obs asks)."""
        from .frame_dir import LoadedSplit, SplitPlan, episode_table

        c = self.dataset_cfg
        kw = dict(cameras=self.cams, action_type=c.get("action_type", "rel_actions_world"), n_digits=c.get("n_digits"),
                  real_world=bool(c.get("real_world", False)), store_size=c.get("store_size"), cache_dir=c.get("cache_dir"),
                  workers=c.get("workers", 8), chunk_frames=c.get("chunk_frames", 256), ring=c.get("ring", 3))
        want_val = self.val_percentage > 0 and self._dirs["validation"] is not None
        names = ("train", "validation") if want_val else ("train",)
        self.splits = {}
        if self._one_dir and want_val:
            # one directory, one array: its rows are the steps either table covers, and each split's table is remapped to them
            eps = {s: episode_table(self._dirs[s], s) for s in names}
            ep = np.concatenate(list(eps.values()))
            plan = SplitPlan(self._dirs["train"], "train", want_robot_obs=any(self._want_robot_obs(s) for s in names),
                             episodes=ep[np.argsort(ep[:, 0], kind="stable")], **kw)
            self._settle_resize(plan.stored)
            whole = plan.load(dev)
            self.load_stats["train"] = plan.stats
            for s in names:
                self.splits[s] = LoadedSplit(whole.frames, whole.actions, whole.rows(eps[s]), whole.step_of_row,
                                             whole.robot_obs, whole.root, s)
        else:
            plans = {s: SplitPlan(self._dirs[s], s, want_robot_obs=self._want_robot_obs(s), **kw) for s in names}
            self._settle_resize(plans["train"].stored)
            for s, plan in plans.items():  # (every split's refusals came first)
                self.splits[s] = plan.load(dev)
                self.load_stats[s] = plan.stats
        out = [(d.frames, d.actions, d.ep) for d in (self.splits["train"], self.splits.get("validation")) if d is not None]
        return out[0], (out[1] if len(out) > 1 else None)

    def _want_robot_obs(self, split):
        """Whether the split's robot_obs is loaded beside its frames (a subclass that builds a neighbour table asks)."""
        return False

    def prepare_data(self, *args, **kwargs):
        pass

    def setup(self, stage=None):
        if self.train_replay is not None:
            return
        from ..lightning import default_device

        dev = torch.device(self.device if self.device is not None else default_device())  # one process per GPU
        if "frame_dir" in self.dataset_cfg:
            tr, va = self._frame_dir_splits(dev)
        else:
            frames, actions, ep_train, ep_val = self._arrays()
            frames = {c: torch.as_tensor(v).to(dev).contiguous() for c, v in frames.items()}  # both splits share the frames
            acts = torch.as_tensor(np.asarray(actions, dtype=np.float32)).to(dev)
            tr, va = (frames, acts, ep_train), (frames, acts, ep_val)
        self._settle_resize({c: tuple(v.shape[1:3]) for c, v in tr[0].items()})
        specs = {c: s for c, s in self.aug_specs.items() if s is not None and (s.resize is not None or s.pad or s.prob)}
        self._train_specs = specs or None
        self.index = ix = self._index(tr[2], self.train_percentage, "train", self._n_frames(tr[0], tr[1]), dev)
        self.train_replay = self._replay(tr[0], tr[1], ix, dev)
        if self.val_percentage > 0:
            if va is None or va[2] is None:
                raise KeyError(f"{type(self).__name__}: val_percentage > 0 needs `ep_start_end_ids_val`")
            vix = self._index(va[2], self.val_percentage, "validation", self._n_frames(va[0], va[1]), dev)
            self.val_replay = self._replay(va[0], va[1], vix, dev)
            if self.val_steps is None:
                self.val_steps = max(len(vix) // self.batch_size, 1)
        if self.steps_per_epoch is None:
            self.steps_per_epoch = len(ix) // self.batch_size
        if int(self.steps_per_epoch) < 1:
            raise ValueError(f"{len(ix)} items give no batch of {self.batch_size}")

    def train_dataloader(self):
        self.setup()
        return self.LOADER(self.train_replay, self.batch_size, self.steps_per_epoch, aug_specs=self._train_specs,
                           generator=self.generator, fused=self.fused)

    def val_dataloader(self):
        self.setup()
        if self.val_replay is None:
            return None
        return self.LOADER(self.val_replay, self.batch_size, self.val_steps, generator=self.generator, train=False,
                           fused=self.fused)
