"""The neighbour table of the `similar_robot_obs` goal strategy, built on the device.

The reference builds `nn_steps_from_step` once per dataset (set_nn_steps_from_step: datamodule/dataset/play_dataset.py:183-234,
goal_cond_replay_buffer_dataset.py:76-130) with faiss.IndexFlatL2: an exact brute-force L2 search of every frame's robot_obs
for its num_nn = 32 nearest frames, then a temporal filter that drops neighbours closer than margin = 16 steps.  Here the
search is `tacorl_knn_l2` and the filter `tacorl_nn_margin_filter` (csrc/knn_ops.hip); the definition both follow is in
include/tacorl_hip.h and restated in NumPy by `nn_steps_from_step_host`:

* the searched rows are the frames range(start, end) of every episode in order - the episodes' inclusive end steps are
  left out, as in the reference loop - so step ids ascend but are not contiguous;
* d(q, p) in fp32, sequentially over the columns, acc = acc + (q_j - p_j) * (q_j - p_j), each operation rounded once;
* the neighbours of a row are the min(num_nn, N) rows with the smallest (d, row), the query's own row included;
* AFTER the top-k, neighbour step s of query step t is dropped iff |t - s| < margin (pure id arithmetic, across episode
  boundaries); survivors keep their distance order.  Most of a trajectory's nearest frames are its temporal neighbours, so
  lists are short and often empty - the samplers' fallback to a random state relies on that.

`NeighbourTable` holds the result as the CSR (ptr, val) indexed by frame id that PlayIndex, TransitionIndex and the device
samplers use, and reads / writes the reference's JSON file."""
import json
import os

import numpy as np
import torch

from .. import ops

MAX_D, MAX_K = ops.KNN_MAX_D, ops.KNN_MAX_K


def _episodes(ep_start_end_ids, n_frames):
    """The checks of TransitionIndex: sorted, non-overlapping, inside the array."""
    ep = np.asarray(ep_start_end_ids, dtype=np.int64).reshape(-1, 2)
    if len(ep) == 0:
        raise ValueError("no episodes")
    if ep.min() < 0 or ep.max() >= n_frames:
        raise ValueError(f"episode bounds outside [0, {n_frames})")
    if (ep[:, 0] > ep[:, 1]).any() or (ep[1:, 0] <= ep[:-1, 1]).any():
        raise ValueError("episodes must be sorted by start and must not overlap")
    return ep


def _searched_steps(ep):
    """range(start, end) per episode: the end step is no query and no candidate (reference :101-105)."""
    steps = np.concatenate([np.arange(s, e) for s, e in ep])
    if len(steps) == 0:
        raise ValueError("no step to search: every episode is a single frame")
    if len(steps) > 2**31 - 1:
        raise ValueError("more than 2^31 - 1 rows")
    return steps


def _check_sizes(D, num_nn, margin):
    if not 1 <= int(D) <= MAX_D:
        raise ValueError(f"robot_obs has {D} columns; supported: 1..{MAX_D}")
    if not 1 <= int(num_nn) <= MAX_K:
        raise ValueError(f"num_nn {num_nn} outside 1..{MAX_K}")
    if int(margin) < 0:
        raise ValueError(f"margin {margin} is negative")


class NeighbourTable:
    """nn_steps_from_step as a CSR indexed by frame id: the neighbours of step s are val[ptr[s]:ptr[s + 1]], in distance
    order.  ptr int64 (n_frames + 1), val int64, steps int64 = the searched steps (the keys of the reference's dict: they
    include steps whose list is empty, and no episode end step), ascending; all three on one device."""

    def __init__(self, ptr, val, steps, n_frames):
        self.ptr, self.val, self.steps, self.n_frames = ptr, val, steps, int(n_frames)
        assert ptr.dtype == val.dtype == steps.dtype == torch.int64 and ptr.numel() == self.n_frames + 1
        assert ptr.device == val.device == steps.device
        self._host = None

    @property
    def device(self):
        return self.ptr.device

    def to(self, device):
        device = torch.device(device)
        if device == self.ptr.device:
            return self
        return NeighbourTable(self.ptr.to(device), self.val.to(device), self.steps.to(device), self.n_frames)

    def host(self):
        """(ptr, val, steps) as NumPy arrays (copied from the device once)."""
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in (self.ptr, self.val, self.steps))
        return self._host

    def index_csr(self):
        """(ptr, val) as the sampling indices keep them: ptr cut behind the last searched step, as it comes out of a dict."""
        ptr, val, steps = self.host()
        top = int(steps[-1]) + 1 if len(steps) else 0
        return ptr[: top + 1], val

    @classmethod
    def from_dict(cls, nn_steps_from_step, n_frames, device="cpu"):
        keys = np.array(sorted(int(k) for k in nn_steps_from_step), dtype=np.int64)
        if len(keys) and (keys[0] < 0 or keys[-1] >= n_frames):
            raise ValueError(f"nn_steps_from_step: a step outside [0, {n_frames})")
        lists = {int(k): v for k, v in nn_steps_from_step.items()}
        cnt = np.zeros(int(n_frames), dtype=np.int64)
        cnt[keys] = [len(lists[int(k)]) for k in keys]
        ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        val = np.concatenate([np.asarray(lists[int(k)], dtype=np.int64).reshape(-1) for k in keys] + [np.zeros(0, np.int64)])
        dev = torch.device(device)
        return cls(torch.from_numpy(ptr).to(dev), torch.from_numpy(val).to(dev), torch.from_numpy(keys).to(dev), n_frames)

    def to_dict(self):
        """{int step: [int, ...]} with a key for every searched step (empty lists included, end steps absent)."""
        ptr, val, steps = self.host()
        return {int(s): val[ptr[s]:ptr[s + 1]].tolist() for s in steps}

    def save_json(self, path, data_type="train"):
        """Merge into the reference's file {"train": {...}, "validation": {...}} (string keys, indent=4), as
        set_nn_steps_from_step writes it: the unmodified reference reads the result."""
        path = os.path.expanduser(str(path))
        doc = {}
        if os.path.isfile(path):
            with open(path) as f:
                doc = json.load(f)
        doc[data_type] = {str(k): v for k, v in self.to_dict().items()}
        tmp = f"{path}.tmp{os.getpid()}"  # (renamed when complete: a process that starts meanwhile never reads half a file)
        with open(tmp, "w") as f:
            json.dump(doc, f, indent=4)
        os.replace(tmp, path)

    @classmethod
    def load_json(cls, path, data_type, n_frames, device="cpu"):
        with open(os.path.expanduser(str(path))) as f:
            doc = json.load(f)
        if data_type not in doc:
            raise KeyError(f"{path}: no '{data_type}' table (has: {sorted(doc)})")
        return cls.from_dict({int(k): v for k, v in doc[data_type].items()}, n_frames, device)


def _host_array(robot_obs):
    a = robot_obs.detach().cpu().numpy() if torch.is_tensor(robot_obs) else np.asarray(robot_obs)
    if a.ndim != 2:
        raise ValueError(f"robot_obs must be (n_frames, D), got {a.shape}")
    return a


def nn_steps_from_step_host(robot_obs, ep_start_end_ids, num_nn=32, margin=16, block=256):
    """The definition in NumPy, for machines without a GPU (and the tests' restatement of the kernels): fp32 arithmetic in
    the kernel's order, `block` queries at a time, a stable argsort for the (distance, row) order.  Returns the reference's
    dict {step: [neighbour steps]}."""
    pts, steps = _points_host(robot_obs, ep_start_end_ids, num_nn, margin)
    rows, _ = knn_l2_host(pts, num_nn, block)
    out = {}
    for i, t in enumerate(steps):
        s = steps[rows[i][rows[i] >= 0]]
        out[int(t)] = s[np.abs(s - t) >= margin].tolist()
    return out


def _points_host(robot_obs, ep_start_end_ids, num_nn, margin):
    a = _host_array(robot_obs)
    _check_sizes(a.shape[1], num_nn, margin)
    steps = _searched_steps(_episodes(ep_start_end_ids, a.shape[0]))
    pts = np.ascontiguousarray(a[steps], dtype=np.float32)
    if not np.isfinite(pts).all():
        raise ValueError("robot_obs holds non-finite values")
    return pts, steps


def knn_l2_host(points, k, block=256, q0=0, n_queries=None):
    """(rows (n_queries, k) int32, distances (n_queries, k) fp32): the search of tacorl_knn_l2 restated in NumPy, for the
    query rows [q0, q0 + n_queries) (default: all)."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    N, D = pts.shape
    nq = N - q0 if n_queries is None else int(n_queries)
    kk = min(int(k), N)
    rows = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    with np.errstate(over="ignore"):
        for b in range(0, nq, block):
            q = pts[q0 + b:q0 + min(b + block, nq)]
            acc = np.zeros((len(q), N), dtype=np.float32)
            for j in range(D):
                t = q[:, j, None] - pts[None, :, j]
                acc = acc + t * t
            order = np.argsort(acc, axis=1, kind="stable")[:, :kk]
            rows[b:b + block, :kk] = order
            dist[b:b + block, :kk] = np.take_along_axis(acc, order, axis=1)
    return rows, dist


def build_nn_steps_from_step(robot_obs, ep_start_end_ids, num_nn=32, margin=16, device=None, query_block=None):
    """robot_obs (n_frames, D), indexed by frame id (array or tensor, on any device); ep_start_end_ids (E, 2) inclusive.
    Searches on `device` (default: the current GPU), `query_block` query rows per launch pair (default 2^18: the temporary
    (rows, steps) lists of a slice stay at 96 MB for num_nn = 32).  Returns the NeighbourTable on that device."""
    if not torch.is_tensor(robot_obs):
        robot_obs = _host_array(robot_obs)
    if robot_obs.ndim != 2:
        raise ValueError(f"robot_obs must be (n_frames, D), got {tuple(robot_obs.shape)}")
    n_frames, D = robot_obs.shape
    _check_sizes(D, num_nn, margin)
    steps_h = _searched_steps(_episodes(ep_start_end_ids, n_frames))
    if torch.is_tensor(robot_obs):
        pts = robot_obs[torch.from_numpy(steps_h).to(robot_obs.device)].to(torch.float32)
        finite = bool(torch.isfinite(pts).all())
    else:
        pts = torch.from_numpy(np.ascontiguousarray(robot_obs[steps_h], dtype=np.float32))
        finite = bool(np.isfinite(pts.numpy()).all())
    if not finite:
        raise ValueError("robot_obs holds non-finite values")
    # everything above is validation and runs without a device
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("build_nn_steps_from_step runs on the GPU; nn_steps_from_step_host is the NumPy form")
    pts, steps = pts.to(dev).contiguous(), torch.from_numpy(steps_h).to(dev)
    N, k = pts.shape[0], int(num_nn)
    qb = min(N, int(query_block) if query_block else 1 << 18)
    if qb < 1:
        raise ValueError(f"query_block {query_block} must be positive")
    rows = torch.empty(qb, k, dtype=torch.int32, device=dev)
    nn_steps = torch.empty(qb, k, dtype=torch.int64, device=dev)
    cnt_row = torch.empty(N, dtype=torch.int32, device=dev)
    vals = []
    for q0 in range(0, N, qb):
        n = min(qb, N - q0)
        ops.knn_l2(pts, k, q0, n, nbr_row=rows[:n], want_dist=False)
        ops.nn_margin_filter(rows[:n], steps, margin, q0, nn_steps=nn_steps[:n], count=cnt_row[q0:q0 + n])
        vals.append(nn_steps[:n][nn_steps[:n] >= 0])  # row-major: the queries in step order, each list in distance order
    cnt = torch.zeros(n_frames, dtype=torch.int64, device=dev)
    cnt[steps] = cnt_row.to(torch.int64)
    ptr = torch.zeros(n_frames + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=ptr[1:])
    return NeighbourTable(ptr, torch.cat(vals), steps, n_frames)
