"""The reference's dataset directory read into resident replay (the dataset key `frame_dir` of the frame datamodules).

The reference's PlayDataset (datamodule/dataset/play_dataset.py) and CALVIN keep one compressed .npz per frame, named
`<prefix><step, n_digits wide>.npz` with `rgb_static`, `rgb_gripper`, `rel_actions_world` / `rel_actions_gripper`,
`robot_obs` and `scene_obs`; the episode table in `split.json` or `ep_start_end_ids.npy` (absolute step numbers, inclusive
ends, gaps between episodes, no start at 0) and optionally the neighbour table in `nn_steps_from_step.json`.  Here:

* `FrameDirectory`: one split of such a directory - the tables by the reference's rules (:332-355, 421-446), the compaction
  of the steps the split's episodes cover to rows 0..N-1, the refusals, and `load`, which decodes the frames with a thread
  pool into a ring of pinned chunk buffers and copies each chunk to the device while the next one decodes;
* `SplitPlan` / `load_split`: a split as the arrays a resident replay takes (`LoadedSplit`), through `store_size` (every
  uploaded chunk passes tacorl_resize_frames_u8: only the chunk buffer holds camera-resolution frames on the device) and `cache_dir`
  (the compacted arrays as .npy, memory-mapped and uploaded in chunks by later starts);
* `split_neighbours`: the split's nn_steps_from_step, read from the directory's JSON file or built with
  neighbours.build_nn_steps_from_step on step numbers and written back in the reference's form, remapped to rows.
"""
import hashlib
import json
import os
import pickle
import re
import shutil
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_WORKERS = 16
SPLIT_DIRS = {"train": "training", "validation": "validation"}


def split_dirs(frame_dir):
    """{"train": dir, "validation": dir or None} and whether the two are one directory: `frame_dir` is a root holding
    training/ and validation/ (what BasicDataModule appends to data_dir), or a single split directory whose split.json holds
    both tables (with ep_start_end_ids.npy alone it has no validation table)."""
    root = os.path.expanduser(str(frame_dir))
    if not os.path.isdir(root):
        raise FileNotFoundError(f"frame_dir {root} is not a directory")
    tr = os.path.join(root, SPLIT_DIRS["train"])
    if os.path.isdir(tr):
        va = os.path.join(root, SPLIT_DIRS["validation"])
        return {"train": tr, "validation": va if os.path.isdir(va) else None}, False
    return {"train": root, "validation": root if os.path.isfile(os.path.join(root, "split.json")) else None}, True


def episode_table(root, split):
    """set_ep_start_end_ids (:421-446): split.json where present - the train key contains "train", the validation key
    "val" - otherwise ep_start_end_ids.npy.  (E,2) int64, absolute inclusive step numbers."""
    sj = os.path.join(root, "split.json")
    if os.path.isfile(sj):
        with open(sj) as f:
            doc = json.load(f)
        want = "train" if split == "train" else "val"
        keys = [k for k in doc if want in k]
        if not keys:
            raise KeyError(f"{sj}: no key containing '{want}' (has: {sorted(doc)})")
        ep = np.asarray(doc[keys[0]], dtype=np.int64).reshape(-1, 2)
    else:
        path = os.path.join(root, "ep_start_end_ids.npy")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{root}: neither split.json nor ep_start_end_ids.npy")
        ep = np.asarray(np.load(path), dtype=np.int64).reshape(-1, 2)
    if len(ep) == 0:
        raise ValueError(f"{root}: the {split} episode table is empty")
    return ep


def _compaction(step_of_row):
    """(first_step, row_of_step) of the ascending steps of the rows: row_of_step[step - first_step], -1 where no row is."""
    first = int(step_of_row[0])
    row_of_step = np.full(int(step_of_row[-1]) - first + 1, -1, dtype=np.int64)
    row_of_step[step_of_row - first] = np.arange(len(step_of_row), dtype=np.int64)
    return first, row_of_step


def _unreadable(path, e):
    return OSError(f"{path}: cannot be read as a frame file ({type(e).__name__}: {e})")


_READ_ERRORS = (OSError, zipfile.BadZipFile, ValueError, pickle.UnpicklingError, EOFError)


def _rows(tab, steps):
    """Step numbers -> rows of the compaction `tab` (row_of_step, first_step); a step that has no row is refused."""
    s = np.asarray(steps, dtype=np.int64)
    k = s - tab.first_step
    ok = (k >= 0) & (k < len(tab.row_of_step))
    r = np.where(ok, tab.row_of_step[np.clip(k, 0, len(tab.row_of_step) - 1)], -1)
    if (r < 0).any():
        raise ValueError(f"{tab.root}: step {int(s[r < 0].flat[0])} lies in no {tab.split} episode")
    return r


class FrameDirectory:
    """One split (`train` / `validation`) of a directory in the reference's layout.  The constructor reads the tables and
    lists the directory; it opens no frame file (`probe()` and `load()` do).  Attributes: `ep_steps` (E,2) absolute inclusive,
    `ep` (E,2) the same in rows, `step_of_row` (N) and `row_of_step` (last - first + 1; -1 where no episode covers the step)
    int64, `first_step`, `n`; `stats` counts the frame files loaded (`files_opened`), the files whose array headers
    check_frames() read (`headers_checked`) and the host chunk buffers allocated - all on the calling thread.
    real_world is the reference's key and has no effect here: there it only drops scene_obs and state_info, which a replay
    never holds.  names: the directory's .npz names where the caller listed it already."""

    def __init__(self, root, split="train", cameras=("rgb_static",), action_type="rel_actions_world", n_digits=None,
                 real_world=False, episodes=None, names=None):
        if split not in SPLIT_DIRS:
            raise ValueError(f"split {split!r}: 'train' or 'validation'")
        self.root, self.split = os.path.expanduser(str(root)), split
        self.cameras, self.action_type, self.real_world = tuple(cameras), str(action_type), bool(real_world)
        if not os.path.isdir(self.root):
            raise FileNotFoundError(f"{self.root} is not a directory")
        self.ep_steps = (episode_table(self.root, split) if episodes is None
                         else np.asarray(episodes, dtype=np.int64).reshape(-1, 2))  # (episodes: the rows of a shared array)
        names = sorted(names) if names is not None else frame_files(self.root)
        if not names:
            raise FileNotFoundError(f"{self.root}: no .npz frame file")
        self.prefix, self.n_digits = name_pattern(self.root, names[0], n_digits)
        self.n_files = len(names)
        ep = self.ep_steps
        if (ep[:, 0] > ep[:, 1]).any() or (ep[1:, 0] <= ep[:-1, 1]).any() or ep.min() < 0:
            raise ValueError(f"{self.root}: episodes must be sorted by start, must not overlap and hold no negative step")
        self.step_of_row = np.concatenate([np.arange(s, e + 1, dtype=np.int64) for s, e in ep])
        self.n = len(self.step_of_row)
        self.first_step, self.row_of_step = _compaction(self.step_of_row)
        self.ep = self.rows(ep)
        have = set(names)
        for s in self.step_of_row:  # a step that an episode names and that has no file
            if os.path.basename(self.file_of(s)) not in have:
                raise FileNotFoundError(f"{self.file_of(s)}: step {int(s)} of the {split} episodes has no frame file")
        self.stats = {"files_opened": 0, "headers_checked": 0, "host_buffers": 0, "host_bytes": 0}
        self._probe = None

    def file_of(self, step):
        """get_episode_name (:349-355)."""
        return os.path.join(self.root, f"{self.prefix}{int(step):0{self.n_digits}d}.npz")

    def rows(self, steps):
        """Step numbers -> rows (same shape); a step no episode of the split covers is refused."""
        return _rows(self, steps)

    @staticmethod
    def _open(path):
        try:
            return np.load(path)
        except _READ_ERRORS as e:
            raise _unreadable(path, e) from e

    def probe(self):
        """The first frame's shapes: {camera: (H,W,3)}, the action width A and robot_obs's width D (None where the file has
        none).  A missing camera or action key is refused with the file name."""
        if self._probe is None:
            path = self.file_of(self.step_of_row[0])
            self.stats["files_opened"] += 1
            with self._open(path) as z:
                missing = [k for k in self.cameras + (self.action_type,) if k not in z.files]
                if missing:
                    raise KeyError(f"{path}: no array named {missing} (has: {sorted(z.files)})")
                shapes = {}
                for c in self.cameras:
                    a = z[c]
                    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                        raise ValueError(f"{path}: {c} must be uint8 (H,W,3), got {a.dtype} {a.shape}")
                    shapes[c] = tuple(a.shape)
                A = int(np.asarray(z[self.action_type]).reshape(-1).shape[0])
                D = int(np.asarray(z["robot_obs"]).reshape(-1).shape[0]) if "robot_obs" in z.files else None
            self._probe = (shapes, A, D)
        return self._probe

    def _check_headers(self, row, want_robot_obs):
        """The .npy headers of one frame file's cameras, action and robot_obs arrays against the first frame's: read from
        the zip members' first bytes, no array is inflated."""
        shapes, A, D = self._probe
        path = self.file_of(self.step_of_row[row])
        want = {c: (shapes[c], np.dtype(np.uint8)) for c in self.cameras}
        want[self.action_type] = (A, None)
        if want_robot_obs:
            want["robot_obs"] = (D, None)
        try:
            with zipfile.ZipFile(path) as z:
                have = set(z.namelist())
                missing = [k for k in want if k + ".npy" not in have]
                if missing:
                    raise KeyError(f"{path}: no array named {missing}")
                for k, (shape, dtype) in want.items():
                    with z.open(k + ".npy") as f:
                        version = np.lib.format.read_magic(f)
                        got, _, dt = (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(f)
                    if dtype is not None and (tuple(got) != tuple(shape) or dt != dtype):
                        raise ValueError(f"{path}: {k} is {dt} {tuple(got)}, the first frame's is {dtype} {tuple(shape)}")
                    if dtype is None and int(np.prod(got, dtype=np.int64)) != shape:
                        raise ValueError(f"{path}: {k} has {int(np.prod(got, dtype=np.int64))} values, the first frame's {shape}")
        except (KeyError, ValueError):
            raise
        except _READ_ERRORS as e:
            raise _unreadable(path, e) from e

    def check_frames(self, workers=8, want_robot_obs=False):
        """Every frame file of the split against the first frame (probe()): a missing camera, action or robot_obs array and a
        frame whose shape or dtype differs are refused with the file name - before load() uploads anything.  Only the
        arrays' headers are read, by the pool load() uses."""
        self.probe()
        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as pool:
            list(pool.map(lambda r: self._check_headers(r, want_robot_obs), range(self.n)))  # (re-raises the first refusal)
        self.stats["headers_checked"] += self.n

    def _decode(self, row, slot, bufs, actions, robot_obs):
        """One frame file into slot `slot` of the chunk buffers and row `row` of the host tables."""
        shapes, A, D = self._probe
        path = self.file_of(self.step_of_row[row])
        with self._open(path) as z:
            missing = [k for k in self.cameras + (self.action_type,) + (("robot_obs",) if robot_obs is not None else ())
                       if k not in z.files]
            if missing:
                raise KeyError(f"{path}: no array named {missing}")
            for c in self.cameras:
                a = z[c]
                if a.shape != shapes[c] or a.dtype != np.uint8:
                    raise ValueError(f"{path}: {c} is {a.dtype} {a.shape}, the first frame's is uint8 {shapes[c]}")
                bufs[c][slot] = a
            act = np.asarray(z[self.action_type], dtype=np.float32).reshape(-1)
            if act.shape[0] != A:
                raise ValueError(f"{path}: {self.action_type} has {act.shape[0]} values, the first frame's {A}")
            actions[row] = act
            if robot_obs is not None:
                ro = np.asarray(z["robot_obs"], dtype=np.float32).reshape(-1)
                if ro.shape[0] != robot_obs.shape[1]:
                    raise ValueError(f"{path}: robot_obs has {ro.shape[0]} values, the first frame's {robot_obs.shape[1]}")
                robot_obs[row] = ro

    def load(self, out, workers=8, chunk_frames=256, ring=3):
        """Fills out["frames"][camera] (N,h,w,3) uint8 tensors (on any device), out["actions"] (N,A) and, where given,
        out["robot_obs"] (N,D) float32 NumPy arrays.  Chunks of `chunk_frames` consecutive rows are decoded by a pool of
        min(workers, 16) threads into a ring of `ring` host chunk buffers per camera (pinned where the frames go to a GPU);
        a chunk is copied to the device asynchronously while the next one decodes, so the host memory in use is bounded by
        ring * chunk_frames * frame_bytes, not by the dataset.  Where out's frames are smaller than the files' (store_size),
        the chunk goes through one device chunk buffer and tacorl_resize_frames_u8."""
        shapes, A, D = self.probe()
        source = lambda r0, r1, slot_bufs: self._decode_chunk(r0, r1, slot_bufs, out["actions"], out.get("robot_obs"), pool)  # noqa: E731
        if out.get("robot_obs") is not None and D is None:
            raise KeyError(f"{self.file_of(self.step_of_row[0])}: no array named ['robot_obs']")
        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as pool:
            upload_chunks(self.n, shapes, out["frames"], source, chunk_frames, ring, self.stats)

    def _decode_chunk(self, r0, r1, bufs, actions, robot_obs, pool):
        self.stats["files_opened"] += r1 - r0  # (counted here, on the submitting thread)
        list(pool.map(lambda r: self._decode(r, r - r0, bufs, actions, robot_obs), range(r0, r1)))  # (re-raises a refusal)


def frame_files(root):
    """The names of the directory's .npz files, sorted."""
    return sorted(e.name for e in os.scandir(root) if e.name.endswith(".npz"))


def name_pattern(root, name, n_digits=None):
    """(prefix, digits) of the directory's frame-file names, read off one of them - the reference takes whichever file scandir
    names first: every frame file shares the pattern."""
    stem = name[:-4]
    digits = re.findall(r"\d+", stem)
    if not digits:
        raise ValueError(f"{os.path.join(root, name)}: no step number in the file name")
    nd = int(n_digits) if n_digits is not None else len(digits[0])
    if nd < 1:
        raise ValueError(f"n_digits {nd} < 1")
    return re.split(r"\d+", stem)[0], nd


def step_files(root, n_digits=None):
    """The directory's frame files by step number alone - no episode table - for readers that name single steps (the rollout
    callback's start and goal states): step -> path, by the file-name rule FrameDirectory.file_of applies."""
    root = os.path.expanduser(str(root))
    if not os.path.isdir(root):
        raise FileNotFoundError(f"{root} is not a directory")
    names = frame_files(root)
    if not names:
        raise FileNotFoundError(f"{root}: no .npz frame file")
    prefix, nd = name_pattern(root, names[0], n_digits)
    have = set(names)

    def file_of(step):
        name = f"{prefix}{int(step):0{nd}d}.npz"
        if name not in have:
            raise FileNotFoundError(f"{os.path.join(root, name)}: step {int(step)} has no frame file")
        return os.path.join(root, name)

    return file_of


def _copy_chunk(dst, src, non_blocking):
    """Every byte of a frame that reaches its destination device passes here (the tests count the calls)."""
    dst.copy_(src, non_blocking=non_blocking)


def upload_chunks(n, shapes, frames, source, chunk_frames, ring, stats):
    """The ring of the loader: `source(r0, r1, {camera: host chunk buffer})` fills rows [r0, r1) into a ring slot's buffers
    (NumPy views of pinned memory where the destination is a GPU), which then go to frames[camera][r0:r1] - straight, or
    through a device chunk buffer and the resize kernel where the destination's frame size differs from shapes[camera]."""
    from .. import ops

    chunk_frames, ring = max(1, int(chunk_frames)), max(1, int(ring))
    resized = [c for c, shp in shapes.items() if tuple(frames[c].shape[1:]) != tuple(shp)]
    if any(frames[c][0].numel() % 16 for c in resized):
        # the resize kernel takes a 16-byte aligned destination: 16 frames of any size are a multiple of 16 bytes, so chunks of
        # a multiple of 16 frames start on a boundary of the (aligned) array
        chunk_frames = (chunk_frames + 15) // 16 * 16
    chunk_frames = min(chunk_frames, n)
    dev = next(iter(frames.values())).device
    cuda = dev.type == "cuda"
    slots, events, staging = [], [None] * ring, {}
    for _ in range(ring):
        bufs = {}
        for c, shp in shapes.items():
            t = torch.empty((chunk_frames,) + tuple(shp), dtype=torch.uint8, pin_memory=cuda)
            stats["host_buffers"] += 1
            stats["host_bytes"] += t.numel()
            bufs[c] = t
        slots.append(bufs)
    if resized and not cuda:
        raise NotImplementedError("store_size resizes on the GPU (tacorl_resize_frames_u8): the frames must go to one")
    for c in resized:
        staging[c] = torch.empty((chunk_frames,) + tuple(shapes[c]), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev) if cuda else _Null():
        for k, r0 in enumerate(range(0, n, chunk_frames)):
            r1, s = min(r0 + chunk_frames, n), k % ring
            if events[s] is not None:
                events[s].synchronize()  # the copy that last read this slot is done
            source(r0, r1, {c: t.numpy() for c, t in slots[s].items()})
            for c, t in slots[s].items():
                if c in staging:
                    _copy_chunk(staging[c][: r1 - r0], t[: r1 - r0], True)
                    ops.resize_frames_u8(staging[c][: r1 - r0], frames[c][r0:r1])
                else:
                    _copy_chunk(frames[c][r0:r1], t[: r1 - r0], cuda)
            if cuda:
                events[s] = torch.cuda.Event()
                events[s].record()
        if cuda:
            torch.cuda.current_stream().synchronize()  # the ring's pinned pages are released behind the last copy


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class LoadedSplit:
    """A split as a resident replay takes it: `frames` {camera: uint8 (N,H,W,3) on the device}, `actions` (N,A) float32
    tensor on the device, `ep` (E,2) in rows, `robot_obs` (N,D) NumPy or None, and the compaction (`step_of_row`,
    `first_step`, `row_of_step`)."""

    def __init__(self, frames, actions, ep, step_of_row, robot_obs=None, root=None, split="train"):
        self.frames, self.actions, self.ep, self.robot_obs = frames, actions, np.asarray(ep, dtype=np.int64), robot_obs
        self.step_of_row = np.asarray(step_of_row, dtype=np.int64)
        self.n = len(self.step_of_row)
        self.first_step, self.row_of_step = _compaction(self.step_of_row)
        self.root, self.split = root, split
        self.ep_steps = self.step_of_row[self.ep]

    def rows(self, steps):
        return _rows(self, steps)


def cache_key(root, n_files, split, cameras, store_size, action_type, episodes):
    """The name of a split's cache: the directory, its frame-file count, the split and its episode table, the cameras, the
    action key and store_size."""
    doc = json.dumps([os.path.abspath(root), int(n_files), split, list(cameras), [list(map(int, store_size[c])) if store_size.get(c)
                      else None for c in cameras], action_type, np.asarray(episodes).tolist()])
    return hashlib.sha1(doc.encode()).hexdigest()[:20]


def _stored_hw(store_size, cameras):
    """store_size as {camera: (H, W) or None}: [H, W] for every camera, or a mapping per camera."""
    if store_size is None:
        return {c: None for c in cameras}
    if isinstance(store_size, dict) or hasattr(store_size, "items"):
        bad = [c for c in store_size if c not in cameras]
        if bad:
            raise ValueError(f"store_size names {bad}, the cameras are {list(cameras)}")
        return {c: (tuple(int(v) for v in store_size[c]) if store_size.get(c) is not None else None) for c in cameras}
    hw = tuple(int(v) for v in store_size)
    if len(hw) != 2 or min(hw) < 1:
        raise ValueError(f"store_size {store_size}: [H, W]")
    return {c: hw for c in cameras}


class SplitPlan:
    """One split of the directory on its way to a LoadedSplit, in two steps, so that a datamodule can raise every refusal of
    every split before anything is uploaded: the constructor reads the tables, lists the directory and - unless cache_dir
    holds the split - checks the files (FrameDirectory: a step without a file), the first frame and the array headers of
    every other frame (check_frames: a missing key, a shape that differs from the first frame's); `load(device)` then decodes
    and uploads.  `stored`: {camera: (H, W)} the replay will hold.
    cache_dir: after the first load the compacted arrays are written there as .npy under cache_key(...) - into a temporary
    directory that is renamed when it is complete, so ranks that start together never read each other's half-written
    arrays; a later start memory-maps them, uploads them in chunks and opens no frame file.  episodes: the table to use instead of the split's own
    (the union of both splits where they share one array).  `stats`: the reader's counters after load()."""

    def __init__(self, root, split, cameras, action_type, n_digits=None, real_world=False, store_size=None, cache_dir=None,
                 want_robot_obs=False, workers=8, chunk_frames=256, ring=3, episodes=None):
        self.root, self.split, self.cameras = os.path.expanduser(str(root)), split, tuple(cameras)
        self.hw, self.action_type = _stored_hw(store_size, self.cameras), str(action_type)
        self.want_robot_obs, self.workers, self.chunk_frames, self.ring = bool(want_robot_obs), workers, int(chunk_frames), ring
        ep = episode_table(self.root, split) if episodes is None else np.asarray(episodes, dtype=np.int64).reshape(-1, 2)
        names = frame_files(self.root)
        self.cdir = (os.path.join(os.path.expanduser(str(cache_dir)), cache_key(self.root, len(names), split, self.cameras, self.hw, self.action_type, ep))
                     if cache_dir else None)
        self.stats = {"files_opened": 0, "headers_checked": 0, "host_buffers": 0, "host_bytes": 0, "from_cache": False}
        self.cached = self._complete()
        self.directory = None
        if self.cached:
            self._maps = {c: np.load(os.path.join(self.cdir, f"frames_{c}.npy"), mmap_mode="r") for c in self.cameras}
            self.stored = {c: tuple(m.shape[1:3]) for c, m in self._maps.items()}
        else:
            self.directory = fd = FrameDirectory(self.root, split, self.cameras, self.action_type, n_digits, real_world, ep, names)
            shapes, A, D = fd.probe()
            self._robot = self.want_robot_obs or (self.cdir is not None and D is not None)
            if want_robot_obs and D is None:
                raise KeyError(f"{fd.file_of(fd.step_of_row[0])}: no array named ['robot_obs']")
            fd.check_frames(workers, self._robot)
            self.stored = {c: tuple(self.hw[c] or shapes[c][:2]) for c in self.cameras}

    def _complete(self):
        return bool(self.cdir and os.path.isfile(os.path.join(self.cdir, "done"))
                    and (not self.want_robot_obs or os.path.isfile(os.path.join(self.cdir, "robot_obs.npy"))))

    def load(self, device):
        dev = torch.device(device)
        cameras, cdir, cf = self.cameras, self.cdir, max(1, self.chunk_frames)
        if self.cached:
            maps = self._maps
            n = len(next(iter(maps.values())))
            shapes = {c: tuple(m.shape[1:]) for c, m in maps.items()}
            frames = {c: torch.empty((n,) + shapes[c], dtype=torch.uint8, device=dev) for c in cameras}

            def source(r0, r1, bufs):
                for c in cameras:
                    bufs[c][: r1 - r0] = maps[c][r0:r1]

            upload_chunks(n, shapes, frames, source, cf, self.ring, self.stats)
            self.stats["from_cache"] = True
            ro = np.load(os.path.join(cdir, "robot_obs.npy")) if self.want_robot_obs else None
            return LoadedSplit(frames, torch.from_numpy(np.load(os.path.join(cdir, "actions.npy"))).to(dev),
                               np.load(os.path.join(cdir, "ep.npy")), np.load(os.path.join(cdir, "step_of_row.npy")), ro, self.root, self.split)
        fd = self.directory
        shapes, A, D = fd.probe()
        robot = self._robot
        host = {"actions": np.zeros((fd.n, A), np.float32), "robot_obs": np.zeros((fd.n, D), np.float32) if robot else None}
        host["frames"] = {c: torch.empty((fd.n,) + self.stored[c] + (3,), dtype=torch.uint8, device=dev) for c in cameras}
        fd.load(host, self.workers, cf, self.ring)
        self.stats.update(fd.stats)
        out = LoadedSplit(host["frames"], torch.from_numpy(host["actions"]).to(dev), fd.ep, fd.step_of_row,
                          host["robot_obs"] if self.want_robot_obs else None, self.root, self.split)
        if cdir:
            tmp = f"{cdir}.tmp{os.getpid()}"
            os.makedirs(tmp)
            for c in cameras:
                m = np.lib.format.open_memmap(os.path.join(tmp, f"frames_{c}.npy"), mode="w+", dtype=np.uint8, shape=tuple(out.frames[c].shape))
                for r0 in range(0, fd.n, cf):
                    m[r0:r0 + cf] = out.frames[c][r0:r0 + cf].cpu().numpy()
                m.flush()
                del m
            np.save(os.path.join(tmp, "actions.npy"), host["actions"])
            if host["robot_obs"] is not None:
                np.save(os.path.join(tmp, "robot_obs.npy"), host["robot_obs"])
            np.save(os.path.join(tmp, "ep.npy"), fd.ep)
            np.save(os.path.join(tmp, "step_of_row.npy"), fd.step_of_row)
            np.save(os.path.join(tmp, "row_of_step.npy"), fd.row_of_step)
            with open(os.path.join(tmp, "done"), "w") as f:
                f.write(f"{fd.n}\n")
            try:
                if self._complete():  # another rank finished the same arrays first
                    shutil.rmtree(tmp)
                else:
                    shutil.rmtree(cdir, ignore_errors=True)  # (a cache without `done`, or one without robot_obs: replaced)
                    os.rename(tmp, cdir)
            except OSError:
                shutil.rmtree(tmp, ignore_errors=True)
        return out


def load_split(root, split, cameras, action_type, device, stats=None, **kw):
    """SplitPlan(...).load(device) in one call; stats (a dict) receives the reader's counters."""
    plan = SplitPlan(root, split, cameras, action_type, **kw)
    out = plan.load(device)
    if stats is not None:
        stats.update(plan.stats)
    return out


def split_neighbours(data, device, num_nn=32, margin=16, path=None, build=True):
    """The split's nn_steps_from_step as a NeighbourTable over rows, on `device`.  `path` (default: the directory's
    nn_steps_from_step.json; the datamodules pass the file neighbour_file finds) is read with NeighbourTable.load_json where it holds the split's table ("train" /
    "validation", keyed by step number, as set_nn_steps_from_step :183-234 writes it).  Otherwise, with build=True, it is
    built from the split's robot_obs with build_nn_steps_from_step - on step numbers relative to the first step, so that
    the margin filter sees the step distances the reference's does, gaps between episodes included - and written to `path`
    in the reference's form.  None: no file and build=False."""
    from .neighbours import NeighbourTable, build_nn_steps_from_step

    path = os.path.expanduser(str(path)) if path else os.path.join(data.root, "nn_steps_from_step.json")
    last = int(data.step_of_row[-1])
    tab = None
    if os.path.isfile(path):
        try:
            tab = NeighbourTable.load_json(path, data.split, last + 1)
        except KeyError:
            tab = None
    if tab is None:
        if not build:
            return None
        if data.robot_obs is None:
            raise KeyError(f"{data.root}: building nn_steps_from_step needs robot_obs")
        base, span = data.first_step, last - data.first_step + 1
        ro = np.zeros((span, data.robot_obs.shape[1]), np.float32)
        ro[data.step_of_row - base] = data.robot_obs
        rel = build_nn_steps_from_step(ro, data.ep_steps - base, num_nn=num_nn, margin=margin, device=device)
        z = torch.zeros(base, dtype=torch.int64, device=rel.ptr.device)
        tab = NeighbourTable(torch.cat([z, rel.ptr]), rel.val + base, rel.steps + base, span + base)
        tab.save_json(path, data.split)
    ptr, val, keys = tab.host()
    rows, cnt = data.rows(keys), np.zeros(data.n, dtype=np.int64)
    cnt[rows] = np.diff(ptr)[keys]
    rptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    dev = torch.device(device)
    return NeighbourTable(torch.from_numpy(rptr).to(dev), torch.from_numpy(data.rows(val)).to(dev), torch.from_numpy(rows).to(dev), data.n)


def neighbour_file(frame_dir, split_dir, split, configured=()):
    """Where a split's step-keyed nn_steps_from_step lives: the first existing file among `configured` (a path given as
    nn_steps_from_step, the config's nn_steps_from_step_path), <frame_dir>/nn_steps_from_step.json (the reference's file
    sits beside training/ and validation/) and <split_dir>/nn_steps_from_step.json that holds the split's table.  Returns
    (path, True) for it - or (path, False) for where a built table is written: the configured path whose directory exists,
    else the split's directory."""
    given = [os.path.expanduser(str(p)) for p in configured if p]
    places = given + [os.path.join(os.path.expanduser(str(d)), "nn_steps_from_step.json") for d in (frame_dir, split_dir)]
    for p in places:
        if os.path.isfile(p):
            try:
                with open(p) as f:
                    if split in json.load(f):
                        return p, True
            except ValueError:
                pass
    for p in given:
        if os.path.isdir(os.path.dirname(p) or "."):
            return p, False
    return places[-1], False
