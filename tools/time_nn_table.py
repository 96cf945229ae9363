"""Time the neighbour-table build (tacorl_amd.data.neighbours.build_nn_steps_from_step: tacorl_knn_l2 + tacorl_nn_margin_filter
+ the CSR assembly) on one GPU, next to the stock-op composition of the same search on the same table:

  (a) build_nn_steps_from_step, whole: device events around the call (it ends in the finite-check read-back and the table);
  (b) the search kernel alone over all N queries (ops.knn_l2, rows only);
  (c) the yardstick: blocked torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist") + torch.topk(k, largest=False),
      the block sized so that its (block, N) distance matrix stays under --block-bytes and under 2^24 elements (what one launch
      of that cdist can take).  torch's direct-form cdist spends a workgroup per output element: (c) runs --yardstick-queries
      query rows against the whole table and is scaled by N / queries (it is linear in the queries: every block does the same
      work), and the JSON says so - `yardstick_ms_measured` over `yardstick_queries`, `yardstick_ms_scaled` for N.

Rounds of (b) and (c) alternate in one process; medians and minima are reported.  The table is synthetic play data: episodes
of 2 000 frames, each a slow random walk of a D = 15 robot state (consecutive frames are near-duplicates, as in recordings).
Also counted: the queries whose kernel list equals the yardstick's (the yardstick takes square roots and has its own tie
order, so near-ties may differ).

    python tools/time_nn_table.py [--frames 40000 600000] [--rounds 3] [--out FILE]

Prints one JSON line per size (and appends them to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def play_like(n_frames, D, dev, ep_len=2000, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ep = [[s, min(s + ep_len, n_frames) - 1] for s in range(0, n_frames, ep_len)]
    x = torch.empty(n_frames, D, device=dev)
    for s, e in ep:
        start = torch.rand(1, D, device=dev, generator=g) * 2 - 1
        x[s:e + 1] = start + torch.cumsum(0.01 * torch.randn(e + 1 - s, D, device=dev, generator=g), 0)
    return x, ep


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[40000, 600000])
    ap.add_argument("--dim", type=int, default=15)
    ap.add_argument("--num-nn", type=int, default=32)
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--yardstick-queries", type=int, default=4096)
    ap.add_argument("--block-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nn_table: needs a GPU")
    from tacorl_amd import _lib, ops
    from tacorl_amd.data.neighbours import build_nn_steps_from_step

    dev, k = torch.device("cuda:0"), a.num_nn
    _lib.call("tacorl_hip_init", 0)
    for n_frames in a.frames:
        obs, ep = play_like(n_frames, a.dim, dev)
        steps = torch.cat([torch.arange(s, e, device=dev) for s, e in ep])
        pts = obs[steps].contiguous()
        N = pts.shape[0]
        yq = min(a.yardstick_queries, N)
        # torch's direct-form cdist launches 256 threads per output element and HIP takes at most 2^32 threads per launch: a
        # block of more than 2^24 elements comes back with zeros in it (seen at 512 x 39 980), so the block is also held under that
        block = max(1, min(yq, a.block_bytes // (4 * N), ((1 << 24) - 1) // N))

        def yardstick():
            out = torch.empty(yq, k, dtype=torch.int64, device=dev)
            for b in range(0, yq, block):
                e = min(b + block, yq)
                d = torch.cdist(pts[b:e], pts, compute_mode="donot_use_mm_for_euclid_dist")
                out[b:e] = torch.topk(d, k, dim=1, largest=False, sorted=True).indices
            return out

        rows = torch.empty(N, k, dtype=torch.int32, device=dev)
        kernel = lambda: ops.knn_l2(pts, k, nbr_row=rows, want_dist=False)[0]  # noqa: E731
        build = lambda: build_nn_steps_from_step(obs, ep, k, a.margin, device=dev)  # noqa: E731
        # warm-up of every shape the timed window uses (code objects, the allocator's blocks)
        ops.knn_l2(pts, k, 0, min(N, 4096), want_dist=False)
        yardstick()
        t_kernel, t_yard, t_build = [], [], []
        for _ in range(a.rounds):
            t_kernel.append(timed(kernel)[0])
            ms, y_rows = timed(yardstick)
            t_yard.append(ms)
            ms, tab = timed(build)
            t_build.append(ms)
        same = float((rows[:yq].to(torch.int64) == y_rows).all(dim=1).float().mean())
        cnt = (tab.ptr[1:] - tab.ptr[:-1])[tab.steps]
        med = lambda v: float(np.median(v))  # noqa: E731
        line = {"n_frames": n_frames, "rows": N, "D": a.dim, "num_nn": k, "margin": a.margin, "rounds": a.rounds,
                "build_ms_median": med(t_build), "build_ms_min": min(t_build),
                "kernel_ms_median": med(t_kernel), "kernel_ms_min": min(t_kernel),
                "kernel_us_per_query": med(t_kernel) * 1e3 / N,
                "kernel_pair_rate_per_s": N * N / (med(t_kernel) * 1e-3),
                "yardstick_queries": yq, "yardstick_block": block,
                "yardstick_ms_measured_median": med(t_yard), "yardstick_ms_measured_min": min(t_yard),
                "yardstick_us_per_query": med(t_yard) * 1e3 / yq,
                "yardstick_ms_scaled": med(t_yard) * N / yq,
                "kernel_over_yardstick": med(t_kernel) / (med(t_yard) * N / yq),
                "lists_equal_to_yardstick": same,
                "table_entries": int(tab.val.numel()), "empty_lists": float((cnt == 0).float().mean()),
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del obs, pts, rows, tab, y_rows


if __name__ == "__main__":
    main()
