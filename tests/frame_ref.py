"""The store-time resize (tacorl_resize_frames_u8, csrc/frame_ops.hip) restated in NumPy, and the golden directory of the
frame_dir tests.

`resize_u8(frames, H, W, dtype)`: uint8 (n,Hs,Ws,3) -> uint8 (n,H,W,3) by the sampling rule of csrc/bilinear.h -
  src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out; i0 = floor(src), i1 = i0 + (i0 < in - 1); l1 = src - i0, l0 = 1 - l1;
  v = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)
- then round half to even and clamp to 0..255.  dtype=np.float64 is the definition; dtype=np.float32 evaluates it with every
operation rounded to fp32 in the kernel's order (the library is built without contraction).  `values(...)` returns v itself.

The exact shapes of the tests.  25 -> 16 (scale 25/16) and 8 -> 8 (scale 1): every position is a multiple of 1/32, every
weight and every product with a value <= 255 has far fewer than 24 bits, so fp32 computes v exactly and ties (v = k + 1/2)
are rounded alike.  40 -> 24 has scale 5/3, which fp32 does not hold: positions are (5 d + 1) / 3 and v is a multiple of 1/9.
No multiple of 1/9 is a tie, and the nearest one lies 1/18 from it - four orders of magnitude more than `fp32_bound` - so
the fp32 result rounds as the fp64 one does there too.  tests/test_frame_dir_cpu.py asserts all three on random, all-255 and
checkerboard frames.

`fp32_bound(Hs, Ws)`: the a-priori bound of |v_fp32 - v| for a general ratio, u = 2^-24.  A position: scale carries a relative
u, the product scale * (dst + 0.5) <= in another, the subtraction of 0.5 a third: |d src| <= 3 u in.  l1 = src - i0 is exact,
l0 = 1 - l1 adds u: |d weight| <= (3 in + 1) u per axis.  The weights of an axis sum to 1 and a value is <= 255, so the
weight errors move v by at most 255 * 2 * ((3 Hs + 1) + (3 Ws + 1)) u (v is continuous in the position, so a position that
crosses an integer is covered: the two weights trade places over neighbouring pixels); the four roundings along the
longest path of the sum (product, inner sum, product, outer sum) and the second-order terms add less than 255 * 5 u.
An output may differ from the fp64 result only where v lies closer than this to k + 1/2, and then by 1."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
EXACT_SHAPES = [((40, 40), (24, 24)), ((25, 25), (16, 16)), ((8, 8), (8, 8))]
GENERAL_SHAPES = [((15, 20), (8, 8)), ((21, 13), (9, 7))]
MAX_DIFF_SHARE = 0.005


def fp32_bound(Hs, Ws):
    return 255.0 * (2 * ((3 * Hs + 1) + (3 * Ws + 1)) + 5) * U


def _axis(out, inn, dt):
    scale = dt(inn) / dt(out)
    src = np.maximum(scale * (np.arange(out).astype(dt) + dt(0.5)) - dt(0.5), dt(0))
    i0 = np.minimum(src.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = src - i0.astype(dt)
    return i0, i1, dt(1) - l1, l1


def values(frames, H, W, dtype=np.float64):
    """v of every output value, (n,H,W,3) in `dtype`."""
    dt = np.dtype(dtype).type
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim == 4 and f.shape[3] == 3
    y0, y1, h0, h1 = _axis(H, f.shape[1], dt)
    x0, x1, w0, w1 = _axis(W, f.shape[2], dt)
    p = f.astype(dt)
    w0, w1 = w0[None, None, :, None], w1[None, None, :, None]
    h0, h1 = h0[None, :, None, None], h1[None, :, None, None]
    top = w0 * p[:, y0][:, :, x0] + w1 * p[:, y0][:, :, x1]
    bot = w0 * p[:, y1][:, :, x0] + w1 * p[:, y1][:, :, x1]
    v = h0 * top + h1 * bot
    assert v.dtype == np.dtype(dtype)
    return v


def resize_u8(frames, H, W, dtype=np.float64):
    return np.clip(np.rint(values(frames, H, W, dtype)), 0, 255).astype(np.uint8)  # np.rint: round half to even


def tie_distance(frames, H, W):
    """|v - (k + 1/2)| to the nearest rounding boundary, per output value, in fp64."""
    v = values(frames, H, W, np.float64)
    return np.abs(v - np.floor(v) - 0.5)


def kernel_frames(n, hw, seed, kind="random"):
    """The frames the kernel tests use: uniform random values, all 255, or a one-pixel checkerboard of 0 / 255."""
    h, w = hw
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    if kind == "all255":
        return np.full((n, h, w, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, 3)).copy()



# ------------------------------------------------------------------------------------------ the golden directory
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "frame_dir.npz"))
    return g, json.loads(str(g["cfg"]))


def build_golden_dir(root, table="npy", hw=None, with_nn=True):
    """The directory tests/golden/frame_dir.npz was recorded on (tools/gen_frame_dir_golden.py), rebuilt from its seed;
    hw: other frame sizes on the same steps, actions and tables.  Returns ({step: arrays}, cfg)."""
    from tools.make_frame_dir import make_frame_dir

    g, cfg = golden()
    data = make_frame_dir(str(root), cfg["train_ep"], cfg["val_ep"], tuple(hw or cfg["hw"]), seed=cfg["seed"], table=table)
    if with_nn:
        with open(os.path.join(str(root), "nn_steps_from_step.json"), "w") as f:
            json.dump({"train": json.loads(str(g["nn"]))}, f)
    return data, cfg


def golden_draws(g):
    """The golden's named draws as PlayIndex.sample / HbmPlayReplay.batch take them (idx included)."""
    n = len(g["idx"])
    return {"idx": np.asarray(g["idx"], np.int64), "window_size": np.asarray(g["window_size"], np.int64),
            "strategy": np.asarray(g["strategy"], np.int64), "disp": np.asarray(g["disp_draw"], np.int64),
            "noise_step": np.zeros(n, np.int64), "u_choice": np.asarray(g["u_choice"], np.float64),
            "u_random_state": np.asarray(g["u_choice"], np.float64)}


def dataset_cfg(cfg, **over):
    """The reference's dataset config of the golden (config/datamodule/dataset/tacorl.yaml with the golden's sizes)."""
    ds = {"_target_": "tacorl.datamodule.dataset.play_dataset.PlayDataset", "_recursive_": False,
          "modalities": cfg["cameras"] + ["rel_actions_world", "robot_obs", "scene_obs"], "action_type": cfg["action_type"],
          "min_window_size": cfg["min_ws"], "max_window_size": cfg["max_ws"], "pad": True, "include_goal": True,
          "goal_sampling_prob": cfg["p"], "goal_strategy_prob": cfg["strategy"], "data_dir": "~/tacorl/calvin"}
    ds.update(over)
    return ds
