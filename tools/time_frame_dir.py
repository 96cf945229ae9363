"""Time the `frame_dir` loader and the store-time resize kernel on the GPU and write profiles/frame_dir.md.

    python tools/time_frame_dir.py [--frames 3000] [--hw 200 200] [--store 128 128] [--out profiles/frame_dir.md]

A synthetic directory in the reference's layout (tools/make_frame_dir.py: one compressed .npz per frame with both cameras,
both action forms, robot_obs and scene_obs; smooth frames, which compress like camera frames) is written to a temporary
directory; writing it is not timed.  Timed, each with a host clock around work that ends in a device synchronise:

* the first load (frame_dir.load_split: decode by a thread pool into the pinned ring, chunk copies, `store_size` resize)
  at 1, 4 and 16 workers;
* the cached load (the .npy arrays of `cache_dir`, memory-mapped and uploaded in chunks);
* the parent's only route on the same frames: np.load of every file into one array per camera, np.savez, then the `path`
  source (np.load of the .npz and the copy to the device);
* the resize kernel alone, by device events, against the HBM copy rate profiles/tsne.md records for this GPU model.
There is no CPU fallback: without a GPU this fails."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.make_frame_dir import CAMERAS, episodes_of, make_frame_dir  # noqa: E402

HBM_TBS = 6.29  # float4 copy out of HBM on this GPU model (profiles/tsne.md)
RING, CHUNK = 3, 256  # the loader's defaults, given explicitly to every timed load


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--hw", type=int, nargs=2, default=(200, 200))
    ap.add_argument("--store", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_dir.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_frame_dir.py measures on the GPU"
    from tacorl_amd import ops
    from tacorl_amd.data import frame_dir as F

    dev, hw, store = torch.device("cuda", 0), tuple(a.hw), tuple(a.store)
    cams = list(CAMERAS)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "training")
        ep = episodes_of(a.frames, 6)
        t0 = time.perf_counter()
        make_frame_dir(d, ep, None, hw, seed=0, table="npy", smooth=True)
        n = sum(e - s + 1 for s, e in ep)
        size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        print(f"wrote {n} frames, {size / 1e6:.0f} MB in {time.perf_counter() - t0:.1f} s (not timed)", flush=True)
        F.load_split(d, "train", cams, "rel_actions_world", dev, workers=16, ring=RING, chunk_frames=CHUNK)  # warm-up: page cache, pinned allocator, kernels
        F.load_split(d, "train", cams, "rel_actions_world", dev, workers=16, store_size=store)
        rows, at16 = [], None
        for what, kw in [(f"first load, {w} worker(s), frames kept at {hw[0]} x {hw[1]}", dict(workers=w)) for w in (1, 4, 16)] + \
                        [(f"first load, {w} worker(s), store_size {store[0]} x {store[1]}", dict(workers=w, store_size=store)) for w in (1, 4, 16)]:
            t, sp = timed(lambda: F.load_split(d, "train", cams, "rel_actions_world", dev, ring=RING, chunk_frames=CHUNK, **kw))
            rows.append((what, t))
            if kw == dict(workers=16, store_size=store):
                at16 = t
            print(what, f"{t:.2f} s", flush=True)
        cache = os.path.join(tmp, "cache")
        t_w, first = timed(lambda: F.load_split(d, "train", cams, "rel_actions_world", dev, workers=16, store_size=store, cache_dir=cache))
        rows.append((f"first load, 16 workers, store_size, writing cache_dir", t_w))
        st = {}
        t_c, cached = timed(lambda: F.load_split(d, "train", cams, "rel_actions_world", dev, store_size=store, cache_dir=cache, stats=st))
        assert st["from_cache"] and st["files_opened"] == 0 and all(torch.equal(cached.frames[c], first.frames[c]) for c in cams)
        rows.append((f"cached load (memory-mapped .npy at {store[0]} x {store[1]}, chunked upload)", t_c))
        cache2 = os.path.join(tmp, "cache_full")
        F.load_split(d, "train", cams, "rel_actions_world", dev, workers=16, cache_dir=cache2)
        t_c2, _ = timed(lambda: F.load_split(d, "train", cams, "rel_actions_world", dev, cache_dir=cache2))
        rows.append((f"cached load (memory-mapped .npy at {hw[0]} x {hw[1]}, chunked upload)", t_c2))

        # the parent's route: every file into one host array, np.savez, then the `path` source
        def convert():
            fd = F.FrameDirectory(d, "train", cams)
            arr = {c: np.empty((n,) + hw + (3,), np.uint8) for c in cams}
            acts = np.empty((n, 7), np.float32)
            for r, s in enumerate(fd.step_of_row):
                with np.load(fd.file_of(s)) as z:
                    for c in cams:
                        arr[c][r] = z[c]
                    acts[r] = z["rel_actions_world"]
            np.savez(os.path.join(tmp, "play.npz"), actions=acts, ep_start_end_ids_train=fd.ep, **{"frames/" + c: v for c, v in arr.items()})

        def path_source():
            with np.load(os.path.join(tmp, "play.npz")) as z:
                return {c: torch.as_tensor(z["frames/" + c]).to(dev) for c in cams}, torch.as_tensor(z["actions"]).to(dev)

        t_conv, _ = timed(convert)
        t_path, _ = timed(path_source)
        rows.append(("parent route: np.load of each file into one array + np.savez (once)", t_conv))
        rows.append(("parent route: the `path` source (np.load of the .npz + copy to the device, every start)", t_path))

    # the kernel alone
    nk = 2048
    src = torch.randint(0, 256, (nk,) + hw + (3,), dtype=torch.uint8, device=dev)
    out = torch.empty((nk,) + store + (3,), dtype=torch.uint8, device=dev)
    cp = torch.empty_like(src)
    for _ in range(3):
        ops.resize_frames_u8(src, out)
        cp.copy_(src)
    ts, tc = [], []
    for _ in range(20):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(); ops.resize_frames_u8(src, out); e[1].record()
        e[2].record(); cp.copy_(src); e[3].record()
        torch.cuda.synchronize()
        ts.append(e[0].elapsed_time(e[1])); tc.append(e[2].elapsed_time(e[3]))
    ms, mc = float(np.median(ts)), float(np.median(tc))
    moved = src.numel() + out.numel()
    gbs, cgbs = moved / ms / 1e6, 2 * src.numel() / mc / 1e6

    lines += ["# Loading the reference's per-frame directory (`frame_dir`) and the store-time resize", "",
              f"`python tools/time_frame_dir.py --frames {a.frames}` on one MI355X.",
              f"Synthetic directory: {n} frames, two cameras of {hw[0]} x {hw[1]}, one `savez_compressed` file per frame, {size / 1e6:.0f} MB on disk",
              "(smooth frames with a little noise; page cache warm - every row reads the same files).  Host clock around the whole call,",
              "which ends in a device synchronise; one run per row after one warm-up load, so differences of a few percent mean nothing.", "",
              "| what | seconds | frames / s |", "|---|---|---|"]
    lines += [f"| {w} | {t:.2f} | {n / t:.0f} |" for w, t in rows]
    best = min(rows[:3], key=lambda r: r[1])
    lines += ["", f"Host memory of the loader: ring {RING} x {CHUNK} frames x {hw[0] * hw[1] * 3} B x {len(cams)} cameras = "
              f"{RING * CHUNK * hw[0] * hw[1] * 3 * len(cams) / 1e6:.0f} MB pinned, whatever the dataset's size;",
              f"the parent route holds the whole dataset in host memory twice (the arrays, then np.load of the .npz): {2 * n * hw[0] * hw[1] * 3 * 2 / 1e6:.0f} MB here.", "",
              "## tacorl_resize_frames_u8 alone", "",
              f"{nk} frames {hw[0]} x {hw[1]} -> {store[0]} x {store[1]}, device events, median of 20 after 3 warm-up launches: {ms:.3f} ms",
              f"(min {min(ts):.3f}, max {max(ts):.3f}) for {moved / 1e6:.0f} MB read + written = **{gbs:.0f} GB/s**, "
              f"{100 * gbs / 1e3 / HBM_TBS:.1f} % of the {HBM_TBS} TB/s float4 copy rate profiles/tsne.md records for this GPU model;",
              f"a torch copy of the same source in the same loop: {mc:.3f} ms = {cgbs:.0f} GB/s (read + written).",
              f"Per frame the kernel is {100 * (ms / 1e3 / nk) * (n / at16):.2f} % of the 16-worker load with store_size: a first load is bound by the host.",
              "", "## Reading the table", "",
              f"Fastest first load: {best[0]} ({n / best[1]:.0f} frames / s) against {n / t_conv:.0f} frames / s for the conversion to one .npz.",
              "More workers help only as far as the decode runs outside the interpreter lock: zlib's inflate releases it, the zip",
              "directory, the array headers and the copy into the ring hold it.  The first-load rows include the pooled header pass over",
              "every file that comes before the first upload.  The cached loads read arrays written moments before, from the page",
              "cache: they say that the chunked upload costs little beside the decode, not what a cold disk delivers."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
