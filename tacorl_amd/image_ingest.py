"""The image-ingest stage of a training step, stated once for TACORL, PlayLMP, CQL_Offline and RelayImitationLearning: what
kind of image batch has arrived (the batch form), what is to be packed where (pack jobs), and which `tacorl_pack_images*`
entry point packs it (`pack`, the only place that chooses).  It ends at the encoders' NHWC image buffers, where
encoder_stage.py begins; everything here takes device tensors.  Forms: "f32_nchw" (the reference's transformed frames),
"f32_nhwc", "u8" (the dataset's uint8 HWC frames, normalised by the pack: ToTensor + Normalize(0.5, 0.5), bit-identical to the
host-transformed fp32 route, a quarter of the bytes) and "u8_indexed" (a `batch["replay"]`: the resident uint8 dataset and an id
table, gathered and packed in one pass).  Only the uint8 forms take `batch["aug"]`."""
import ctypes as C
from collections import namedtuple

import torch

from . import ops
from ._lib import call
from .encoder_stage import image_flag

U8_FORMS = ("u8", "u8_indexed")


PackJob = namedtuple("PackJob", ops.JOB_FIELDS, defaults=(None, 1, None, None))  # src, pitch, dst, n, index, stride, shift, jitter
PackJob.__doc__ = """n images from src into the NHWC image buffer at dst.  src, dst and index are raw device addresses.
pitch: distance between two source images (for an indexed job: the size of one dataset frame) in ELEMENTS of the source - fp32
values for the f32 forms, bytes for the uint8 forms.  index (None: image i is the i-th image at src): a device int64 table,
image i is dataset frame index[i * stride].  shift (n,2) int32 / jitter (n,8) f32: the per-image augmentation tables (device
tensors, None: that stage is off)."""

# Per camera: src_hw = the frames as stored, hw = the images the encoders see (`aug["resize"]` applied), frames = the image
# tensors (the dataset, for "u8_indexed"); aug: uint8 forms only; T: play windows only; ids: "u8_indexed" only.
BatchForm = namedtuple("BatchForm", "form B T src_hw hw aug frames ids")


def _form(first, nchw, B, T, frames, aug, ids=None):
    if ids is not None:
        form = "u8_indexed"
    else:
        form = "u8" if first.dtype == torch.uint8 else ("f32_nchw" if nchw else "f32_nhwc")  # (uint8 implies HWC)
    at = slice(-2, None) if form == "f32_nchw" else slice(-3, -1)
    src_hw = {c: tuple(v.shape[at]) for c, v in frames.items()}
    hw = src_hw  # the frames as stored; an augmentation spec with a Resize stage sets the encoders' geometry
    rs = (aug or {}).get("resize") or {}
    if rs:
        if form not in U8_FORMS:
            raise ValueError("aug['resize'] needs the dataset's uint8 frames (the resize is part of the uint8 pack)")
        hw = {c: tuple(rs.get(c, src_hw[c])) for c in src_hw}
    return BatchForm(form, B, T, src_hw, hw, aug if form in U8_FORMS else None, frames, ids)


def window_form(batch, nchw=True):
    """A play-window batch (TACORL, PlayLMP): states (B,T,3,H,W) [nchw] or (B,T,H,W,3) per camera, or `batch["replay"]` -
    frames by index out of a uint8 dataset (data/replay.py HbmReplay.batch(fused=True)): B and T come with the id table
    [B*T window frames | B goal frames]."""
    rp = batch.get("replay")
    if rp is not None:
        B, T, ids = rp["B"], rp["T"], rp["ids"]
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == B * T + B
        return _form(None, False, B, T, rp["frames"], batch.get("aug"), ids)
    first = next(iter(batch["states"].values()))
    return _form(first, nchw, *first.shape[:2], batch["states"], batch.get("aug"))


def transition_form(images, nchw=True, aug=None, replay=None, rows=3):
    """A transition batch (CQL_Offline, RelayImitationLearning).  images: per camera one of its (B,3,H,W) [nchw] or
    (B,H,W,3) tensors - the first camera's decides the form - or, with `replay` (data/replay.py HbmTransitionReplay
    .batch(fused=True)), the camera's dataset; the id table is then (3, B): [step | step + 1 | goal] - or, with rows=4
    (data/relay_replay.py HbmRelayReplay), (4, B): [obs | low_level_goal | high_level_goal | high_level_action]."""
    if replay is not None:
        B, ids = replay["B"], replay["ids"]
        if not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == rows * B):
            raise ValueError("transition replay batch: ids must be a contiguous device int64 (3, B) table" if rows == 3 else
                             f"replay batch: ids must be a contiguous device int64 ({rows}, B) table")
        return _form(None, False, B, None, images, aug, ids)
    first = next(iter(images.values()))
    return _form(first, nchw, first.shape[0], None, images, aug)


class LazyImages(dict):
    """NHWC image buffers by camera.  A step that feeds the encoder straight from the batch (TACORL's fp32 route) leaves
    part of a buffer unpacked and registers how to fill it (`defer`); whoever then READS the buffer by name - a test, a
    per-layer fallback, a tool - gets it filled first, so the buffers mean what they always meant.  The step's own launches
    take `raw(c)` (the tensor as it stands) and `drop(c)` what a new batch supersedes."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._pending = {}

    def raw(self, c):
        return dict.__getitem__(self, c)

    def defer(self, c, fill):
        self._pending[c] = fill

    def drop(self, c=None):
        if c is None:
            self._pending.clear()
        else:
            self._pending.pop(c, None)

    def _settle(self, c):
        fill = self._pending.pop(c, None)
        if fill is not None:
            fill()

    def __getitem__(self, c):
        self._settle(c)
        return dict.__getitem__(self, c)

    def values(self):
        return [self[c] for c in self]

    def items(self):
        return [(c, self[c]) for c in self]


# ------------------------------------------------------------------------- augmentation tables
def flat_table(t):
    """A (B,T,k) table of per-frame draws as the window job's (B*T,k)."""
    return None if t is None else t.reshape(-1, t.shape[-1]).contiguous()


def row_table(t, k):
    """The draws of window frame k, (B,k'): the obs / next images of a transition take those of frames 0 / T-1, as in the
    reference, where the transform ran once per window in the dataset."""
    return None if t is None else t[:, k].contiguous()


def window_tables(aug, cam, role, T):
    """The shift / jitter fields of one job of a play-window batch: role "window" (all B*T frames), "obs" / "next" (window
    frames 0 / T - 1) or "goal" (the goal frame's own draws)."""
    if aug is None:
        return {}
    t = aug["goal" if role == "goal" else "states"][cam]
    pick = {"window": flat_table, "obs": lambda x: row_table(x, 0), "next": lambda x: row_table(x, T - 1), "goal": lambda x: x}[role]
    return {"shift": pick(t.get("shift")), "jitter": pick(t.get("jitter"))}


# ------------------------------------------------------------------------------------ dispatch
def vector_ok(jobs, form, hw):
    """The vectorised fp32 pack (ops.pack_images_batch): NCHW, H*W % 4 == 0, 16-byte aligned sources, pitches % 4 == 0."""
    return form == "f32_nchw" and (hw[0] * hw[1]) % 4 == 0 and not any(j.src % 16 or j.pitch % 4 for j in jobs)


def pack(jobs, form, img_dtype, src_hw, hw, aug_pad=None):
    """One camera's jobs into its image buffers, in ONE launch where the form has a batched kernel and the alignment allows:
    uint8 with aug_pad -> ..._u8_resize_aug_gather_batch, "u8_indexed" -> ..._u8_gather_batch, "u8" -> ..._u8_batch (all three:
    frame bytes % 16, 16-byte aligned sources, else an error); "f32_nchw" with vector_ok -> tacorl_pack_images_batch; every
    other fp32 batch falls back to tacorl_pack_images, one launch per job."""
    (H, W), xd = hw, image_flag(img_dtype)
    if form in U8_FORMS:
        fb = 3 * src_hw[0] * src_hw[1]
        if form == "u8_indexed":
            if fb % 16 or any(j.src % 16 for j in jobs):
                raise ValueError("uint8 dataset: H*W*3 must be a multiple of 16 and the tensor 16-byte aligned")
        elif fb % 16 or any(j.src % 16 or j.pitch % 16 for j in jobs):
            raise ValueError("uint8 frames: H*W*3 and the image pitch must be multiples of 16, tensors 16-byte aligned")
        if aug_pad is not None:
            ops.pack_images_u8_resize_aug_batch(jobs, xd, src_hw, H, W, aug_pad)
        elif form == "u8_indexed":
            ops.pack_images_u8_gather_batch(jobs, xd, H, W)
        else:
            ops.pack_images_u8_batch(jobs, xd, H, W)
    elif vector_ok(jobs, form, hw):
        ops.pack_images_batch(jobs, xd, H, W)
    else:
        for j in jobs:
            call("tacorl_pack_images", j.src, j.pitch, int(form == "f32_nchw"), j.dst, xd, j.n, 3, H, W, ops.stream())


def pack_u8_roles(f, cams, X3, slots_of, source_of, img_dtype):
    """uint8 frames into the image slots of every camera in `cams` by the gathering / augmenting pack, one launch per camera
    (CQL_Offline: obs / goal / next; RelayImitationLearning: its four roles).  f: the batch form (f.aug None: the plain
    normalising pack, else f.aug[role][cam] = {"shift", "jitter"} and f.aug["pad"][cam]); slots_of(cam) -> {role: slot of
    X3[cam]} (slot k = image rows [k*B, (k+1)*B)); source_of(cam, role) -> (source address, bytes per source frame, index
    address or None): the dataset and a row of an id table, or a gathered (B,H,W,3) tensor."""
    B, aug = f.B, f.aug
    for c in cams:
        slot = B * 3 * f.hw[c][0] * f.hw[c][1] * X3[c].element_size()  # bytes of one role's packed images
        jobs = []
        for role, k in slots_of(c).items():
            src, fb, ip = source_of(c, role)
            if fb != 3 * f.src_hw[c][0] * f.src_hw[c][1]:
                raise ValueError(f"uint8 frames: camera {c}'s {role} frames are not of the camera's frame size")
            t = aug[role][c] if aug is not None else {}
            jobs.append(PackJob(src, fb, X3[c].data_ptr() + k * slot, B, ip, 1, t.get("shift"), t.get("jitter")))
        pack(jobs, f.form, img_dtype, f.src_hw[c], f.hw[c], aug["pad"][c] if aug is not None else None)


def replay_source(rp, cams, row, what):
    """source_of for a fused replay batch `rp` ({"frames", "ids", "B"}): role -> row of the (rows, B) id table."""
    B, ids, frames = rp["B"], rp["ids"], rp["frames"]
    for c in cams:
        v = frames.get(c)
        if v is None or not (v.is_cuda and v.is_contiguous() and v.dtype == torch.uint8 and v.dim() == 4):
            raise ValueError(f"{what}: camera {c} needs a contiguous device uint8 (N,H,W,3) dataset")
    return lambda c, role: (frames[c].data_ptr(), frames[c][0].numel(), ids.data_ptr() + 8 * B * row[role])


def gathered_source(given, roles):
    """source_of for gathered uint8 tensors given[role][cam] (B,H,W,3): image i of each tensor; roles: {cam: its roles}."""
    for c, rs in roles.items():
        for role in rs:
            t = given[role][c]
            if t.dtype != torch.uint8 or not (t.is_cuda and t.is_contiguous()):
                raise ValueError("batch['aug'] needs the dataset's uint8 frames on the device (the augmentation is part of the uint8 pack)")
    return lambda c, role: (given[role][c].data_ptr(), given[role][c][0].numel(), None)


def pack_window(jobs, T, img_dtype, hw):
    """TACORL's four fp32 jobs [window | obs | goal | next] of a camera that is both a window and an engine camera, where
    vector_ok holds and T >= 2: obs = window frame 0 and next = window frame T - 1 (get_rl_batch) are written from the
    one read of the window; the goal image stays a job of its own."""
    win, obs, goal, nxt = jobs
    ptrs = C.c_void_p * 2
    call("tacorl_pack_images_window_batch", 2, *ops.job_arrays([win, goal], "src", "pitch", "dst", "n"), ptrs(obs.dst, None),
         ptrs(nxt.dst, None), (C.c_int * 2)(T, 0), image_flag(img_dtype), *hw, ops.stream())


def pack_slots(X3, slots, B, hw, srcs, nchw, img_dtype):
    """Images of one camera into slots of its NHWC image buffer X3 (slot i = rows [i*B, (i+1)*B)).  srcs[j] -> slot slots[j]:
    (B,3,H,W) [nchw] or (B,H,W,3) fp32 device tensors, or the dataset's uint8 (B,H,W,3) frames; strided views with a
    uniform image pitch (states[:, 0]) are taken as they are."""
    H, W = hw
    esz, img = X3.element_size(), H * W * 3
    u8 = srcs[0].dtype == torch.uint8
    jobs = []
    for i, t in zip(slots, srcs):
        assert t.is_cuda and t.dtype == (torch.uint8 if u8 else torch.float32) and t[0].is_contiguous() and t.shape[0] == B
        assert tuple(t.shape[-3:]) == ((H, W, 3) if (u8 or not nchw) else (3, H, W)), (tuple(t.shape), (H, W))
        jobs.append(PackJob(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else img, X3.data_ptr() + i * B * img * esz, B))
    pack(jobs, "u8" if u8 else ("f32_nchw" if nchw else "f32_nhwc"), img_dtype, hw, hw)
