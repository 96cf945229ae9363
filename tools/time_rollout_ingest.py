"""Time one policy step of an image rollout from the environments' raw uint8 frames (profiles/rollout_callback.md), for
R in {1, 16, 64} environments, on PlayLMP with 84 x 84 networks fed from 200 x 200 frames (one camera) and with 128 x 128
networks fed from 200 x 200 frames (two cameras), in bf16 (the fused encoder forward) and in f32 (the per-layer path):

  (a) what a caller had to do without FrameIngest: resize and normalise every frame to fp32 CHW on the host (timed apart, as
      `host`), then LatentPlanPolicy.step on the images - the fp32 upload, one pack and one per-layer encoder call per camera
      per network call, the observation encoded twice and the goal once more on a re-planning step;
  (b) FrameIngest + LatentPlanPolicy.step(embeddings=...): the uint8 frames copied into the pinned staging buffers on the host
      (FrameIngest.stage; timed apart too, as `stage`), then one copy per camera, resize and pack on the device, one encoder
      launch per geometry (FrameIngest.submit + encode).

Three kinds of step: `decode` (no row re-plans), `replan` (every row re-plans; (b) has the goal embeddings cached) and
`start` (every row begins an episode: (b) encodes the goals too).

    python tools/time_rollout_ingest.py [--steps 100] [--warmup 10] [--out profiles/rollout_callback.md]

Both paths run in the same process on the same weights and frames, alternating call by call; HIP events around every call
from a synchronised (idle) GPU, so a bracket holds the host's launch path as well; the median of --steps after --warmup with
the 10th and 90th percentile.  `launches`: the library entry points one step calls (torch's own copies and index kernels
are not counted).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (1, 16, 64)
CASES = {"84x84 from 200x200, one camera": (("rgb_static",), (84, 84), (200, 200)),
         "128x128 from 200x200, two cameras": (("rgb_static", "rgb_gripper"), (128, 128), (200, 200))}


def transform_cfg(cams, size):
    lst = [{"_target_": "torchvision.transforms.Resize", "size": list(size)}, {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
           {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]
    return {"transforms": {"validation": {c: list(lst) for c in cams}}}


def host_transform(frames, size):
    """Resize -> ScaleImageTensor -> Normalize(0.5, 0.5) of uint8 (n, Hs, Ws, 3) frames on the host: fp32 (n, 3, H, W)."""
    x = torch.from_numpy(frames).permute(0, 3, 1, 2).float()
    x = torch.nn.functional.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
    return (x / 255 - 0.5) / 0.5


class LaunchCount:
    """Counts the library entry points called while it is active, over every module of the package that holds `call`."""

    def __init__(self):
        import tacorl_amd._lib as L

        self.real, self.n = L.call, 0
        self.mods = [m for name, m in list(sys.modules.items()) if name.startswith("tacorl_amd") and getattr(m, "call", None) is L.call]

    def __enter__(self):
        def counted(name, *a):
            self.n += 1
            return self.real(name, *a)

        for m in self.mods:
            m.call = counted
        return self

    def __exit__(self, *a):
        for m in self.mods:
            m.call = self.real


def bracket(fns, steps, warmup):
    """{name: (median, p10, p90) in us}: the callables - (host preparation or None, the timed part) - alternate, each timed part
    from a synchronised GPU."""
    for _ in range(warmup):
        for prep, f in fns.values():
            if prep is not None:
                prep()
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, (prep, f) in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if prep is not None:
                prep()
            torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    q = lambda v, p: float(np.percentile(v, p))  # noqa: E731
    return {k: (round(q(v, 50), 1), round(q(v, 10), 1), round(q(v, 90), 1)) for k, v in ts.items()}


def case(mod, cams, size, src, R, steps, warmup):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy

    rs = np.random.RandomState(R)
    frames = {c: rs.randint(0, 256, size=(2 * R, *src, 3), dtype=np.uint8) for c in cams}
    raw = [{"observation": {c: frames[c][r] for c in cams}, "goal": {c: frames[c][R + r] for c in cams}} for r in range(R)]
    # (a) the host part, timed apart
    t_host = []
    for _ in range(max(5, steps // 10)):
        t0 = time.perf_counter()
        obs = {c: host_transform(frames[c][:R], size) for c in cams}
        t_host.append(time.perf_counter() - t0)
    goal = {c: host_transform(frames[c][R:], size) for c in cams}
    far = 1 << 30
    pa, pb = LatentPlanPolicy(mod, R, plan_duration=far), LatentPlanPolicy(mod, R, plan_duration=far)
    ing = FrameIngest(mod, R, transform_cfg(cams, size))

    staged = lambda: pb.step(None, None, embeddings=ing.encode(ing.submit()))  # noqa: E731  (the device half of (b))

    def a_decode():
        pa.step(obs, goal)

    def a_replan():
        pa.reset()
        pa.step(obs, goal)

    def b_replan_prep():
        pb.reset()
        ing.stage(raw)

    def b_start_prep():
        pb.reset()
        ing.reset()
        ing.stage(raw)

    arms = {"a_decode": (None, a_decode), "b_decode": (lambda: ing.stage(raw), staged), "a_replan": (None, a_replan),
            "b_replan": (b_replan_prep, staged), "b_start": (b_start_prep, staged)}
    a_replan(), b_start_prep(), staged()
    out = {"host_ms": round(1e3 * float(np.median(t_host)), 2)}
    t_stage = {}
    for k, reset in (("decode", lambda: None), ("start", ing.reset)):  # (b)'s host part: the copy into the pinned buffers
        ts = []
        for _ in range(max(5, steps // 10)):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ing.stage(raw)
            ts.append(time.perf_counter() - t0)
            staged()
        t_stage[k] = round(1e3 * float(np.median(ts)), 2)
    out["stage_ms"] = t_stage
    t = bracket({k: arms[k] for k in ("a_decode", "b_decode")}, steps, warmup)
    t.update(bracket({k: arms[k] for k in ("a_replan", "b_replan", "b_start")}, steps, warmup))
    out["us"] = t
    out["launches"] = {}
    for k, (prep, f) in arms.items():
        if prep is not None:
            prep()
        with LaunchCount() as lc:
            f()
        out["launches"][k] = lc.n
    out["ingest_launches"] = dict(ing.launches)
    # the two paths compute the same step: the embeddings of (b) against the image path on (b)'s own pixels
    emb = ing.step(raw)
    ref = mod.perceptual_encoder.get_state_from_observation(
        {c: ing.images(c)[:R].float().permute(0, 3, 1, 2).contiguous() for c in cams}, list(cams))
    got = torch.cat([emb.obs["lmp"][c] for c in cams], dim=-1)
    out["embedding_relerr"] = float((got - ref).norm() / ref.norm())
    torch.cuda.synchronize()
    return out


def markdown(res):
    L = ["# One policy step of an image rollout from raw uint8 frames", "",
         f"`tools/time_rollout_ingest.py` on {res['device']}: PlayLMP (latent 16, decoder hidden 2048), HIP events around every call "
         f"from a synchronised GPU - a bracket holds the host's launch path too - {res['warmup']} warm-up steps, the median of "
         f"{res['steps']} with the 10th - 90th percentile in brackets, the two paths alternating call by call in one process.  "
         "(a): host resize + normalise to fp32 CHW (the `(a) host` column, not part of (a)'s bracket), then `LatentPlanPolicy.step` on "
         "the images, fp32 upload included; (b): the host's copy of the uint8 frames into the pinned staging buffers (`FrameIngest.stage`, "
         "the `(b) host` column: decoding step / episode start, not part of (b)'s bracket), then `FrameIngest.submit` + `encode` + "
         "`step(embeddings=...)`.  `decode`: no row re-plans; `replan`: every row re-plans ((b): goal embeddings cached); "
         "`start`: every row begins an episode ((a)'s re-planning step is the same work every time, so its `replan` column is its "
         "`start`; its host part there is twice the `(a) host` column, observations and goals).   Times in microseconds unless stated; `launches`: library entry points per step (a) / (b).", ""]
    bad = []
    for name, by_dtype in res["cases"].items():
        for dt, rows in by_dtype.items():
            L += [f"## {name}, {dt}", "",
                  "| R | (a) host, ms | (b) host, ms | (a) decode | (b) decode | b / a | (a) replan | (b) replan | (b) start | start b / a | launches decode | "
                  "launches replan | launches start | start with its host part, ms: a / b | (b) embeddings against the image path |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
            for R, r in rows.items():
                u, n = r["us"], r["launches"]
                f = lambda k: f"{u[k][0]} ({u[k][1]} - {u[k][2]})"  # noqa: E731
                rd, rs = u["b_decode"][0] / u["a_decode"][0], u["b_start"][0] / u["a_replan"][0]
                if rd > 1 or rs > 1 or u["b_replan"][0] > u["a_replan"][0]:
                    bad.append(f"{name}, {dt}, R = {R}")
                L.append(f"| {R} | {r['host_ms']} | {r['stage_ms']['decode']} / {r['stage_ms']['start']} | {f('a_decode')} | {f('b_decode')} | {rd:.2f} | {f('a_replan')} | {f('b_replan')} | "
                         f"{f('b_start')} | {rs:.2f} | {n['a_decode']} / {n['b_decode']} | {n['a_replan']} / {n['b_replan']} | "
                         f"{n['a_replan']} / {n['b_start']} | {2 * r['host_ms'] + u['a_replan'][0] / 1e3:.2f} / "
                         f"{r['stage_ms']['start'] + u['b_start'][0] / 1e3:.2f} | {r['embedding_relerr']:.2g} |")
            L.append("")
    L += ["## The expectation", "",
          "(b)'s step takes no longer than (a)'s at every R, for every kind of step: "
          + ("holds in every row above - FrameIngest is the only route, no row-count switch." if not bad
             else "does NOT hold at " + "; ".join(bad) + ".")]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_callback.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rollout_ingest: needs a GPU")
    from tacorl_amd import _lib
    from tests import cfg_util as C
    from tests import d4rl_cfg as K

    dev = "cuda:0"
    _lib.call("tacorl_hip_init", 0)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "cases": {}}
    for name, (cams, size, src) in CASES.items():
        res["cases"][name] = {}
        for dt in ("bf16", "f32"):
            torch.manual_seed(0)
            mod = K.build(C.playlmp_cfg(cams=cams, device=dev, compute_dtype=dt, image_dtype=dt))
            mod.eval()
            res["cases"][name][dt] = {str(R): case(mod, cams, size, src, R, a.steps, a.warmup) for R in ROWS}
            print(name, dt, json.dumps(res["cases"][name][dt]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
