"""Thin torch-tensor wrappers over the C ABI (device memory + streams are torch's; the
arithmetic is libtacorl_hip.so's).  No function here computes anything itself."""
import ctypes as C

import torch

from . import _lib as L
from ._lib import ACT_NONE, ACT_RELU, ACT_SILU, BF16, F32, call, int_array, ptr, ptr_array, stream  # noqa: F401

import threading

_ws_cache = {}
_alloc_epoch = 0
# Held by a hipGraph capture (modules/common.py GraphMixin._run_segments: warm-up + capture) and by a feeder thread while it
# prepares a batch's device-side tables (data/replay.py prefetching): pinned / device allocations, event synchronisation or
# stream waits issued from another thread during a capture can fail it (hipErrorStreamCaptureUnsupported).  Re-entrant:
# a capture may nest helpers that take it again.
capture_lock = threading.RLock()


def note_alloc():
    """Every (re)allocation of a buffer that a captured hipGraph may hold a raw pointer to - step buffers
    of a new batch shape, a regrown workspace - bumps this epoch.  GraphMixin._run_segments stamps its
    captures with the epoch and drops any capture whose stamp is stale, so a graph is never replayed
    against freed memory (the reference DataLoader has no drop_last: B goes 256 -> r -> 256 every epoch)."""
    global _alloc_epoch
    _alloc_epoch += 1


def alloc_epoch():
    return _alloc_epoch


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag); its address is stable until it has to grow, and
    growing bumps the allocation epoch (captured graphs that point at the old buffer are dropped)."""
    key = (str(device), tag)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = t
        note_alloc()
    return t


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.is_contiguous())
    return t


# ------------------------------------------------------------------------- layouts
def encoder_param_layout():
    off = (C.c_long * 11)()
    total = L.lib().tacorl_encoder_param_layout(off)
    return list(off), int(total)


def encoder_act_layout(n_img, H, W):
    off = (C.c_long * 5)()
    total = L.lib().tacorl_encoder_act_layout(int(n_img), H, W, off)
    if total < 0:
        raise L.TacorlHipError(f"encoder: image {H}x{W} too small for the conv stack")
    return list(off), int(total)


def mlp_param_layout(dims):
    n = len(dims) - 1
    w, b = (C.c_long * n)(), (C.c_long * n)()
    total = L.lib().tacorl_mlp_param_layout(n, int_array(dims), w, b)
    return list(w), list(b), int(total)


def mlp_act_layout(M, dims, acts):
    n = len(dims) - 1
    z, y = (C.c_long * n)(), (C.c_long * n)()
    total = L.lib().tacorl_mlp_act_layout(int(M), n, int_array(dims), int_array(acts), z, y)
    return list(z), list(y), int(total)


# ------------------------------------------------------------------------ primitives
def linear_fwd(xs, ws, bs, act=ACT_NONE, compute=F32, want_z=False):
    M = [x.shape[0] for x in xs]
    K, N = xs[0].shape[1], ws[0].shape[0]
    ys = [torch.empty(m, N, device=xs[0].device) for m in M]
    zs = [torch.empty(m, N, device=xs[0].device) for m in M] if want_z else None
    call("tacorl_linear_fwd", len(xs), ptr_array([_f32(x) for x in xs]), K, ptr_array(ws), ptr_array(bs),
         ptr_array(ys), ptr_array(zs) if zs else None, int_array(M), K, N, act, compute, stream())
    return (ys, zs) if want_z else ys


def conv2d_relu_fwd(xs, ws, bs, stride, compute=F32):
    """xs: NHWC (fp32 or bf16); ws: [CO][KH][KW][CI] fp32."""
    n = [x.shape[0] for x in xs]
    _, H, W, Ci = xs[0].shape
    CO, KH, KW, _ = ws[0].shape
    OH, OW = (H - KH) // stride + 1, (W - KW) // stride + 1
    ys = [torch.empty(k, OH, OW, CO, device=xs[0].device) for k in n]
    xd = BF16 if xs[0].dtype == torch.bfloat16 else F32
    call("tacorl_conv2d_relu_fwd", len(xs), ptr_array(xs), ptr_array(ws), ptr_array(bs), ptr_array(ys),
         int_array(n), H, W, Ci, KH, KW, stride, CO, xd, compute, stream())
    return ys


# --------------------------------------------------------------------------- encoder
def encoder_fwd(imgs, params, outs, acts, H, W, compute=F32):
    n = [i.shape[0] for i in imgs]
    xd = BF16 if imgs[0].dtype == torch.bfloat16 else F32
    call("tacorl_encoder_fwd", len(imgs), ptr_array(imgs), ptr_array(params), ptr_array(outs), ptr_array(acts),
         int_array(n), H, W, xd, compute, stream())


def encoder_bwd_fused_workspace(n, H, W, device, ws_tag):
    """Scratch buffer of the fused encoder backward over problems of n[p] images (its weight-only preparation writes there
    too); None where the LDS-resident backward does not take the geometry / the problem count."""
    nb = L.lib().tacorl_encoder_bwd_fused_ws_bytes(len(n), int_array(n), H, W)
    return workspace(nb, device, ws_tag) if nb else None


def encoder_bwd(imgs, params, acts, d_outs, grads, H, W, compute=F32, accumulate=False, fused=False, n=None, xd=None,
                device=None, ws_tag=None):
    """fused=True: the per-image LDS-resident conv backward (bf16 images + bf16 MFMA + supported geometry).
    imgs: tensors, or raw addresses with n (images per problem), xd (image dtype flag) and device given; ws_tag: the scratch
    buffer's name (steps that may share a process keep their own)."""
    if n is None:
        n, xd, device = [i.shape[0] for i in imgs], BF16 if imgs[0].dtype == torch.bfloat16 else F32, imgs[0].device
    args = [len(imgs), ptr_array(imgs), ptr_array(params), ptr_array(acts), ptr_array(d_outs), ptr_array(grads), int_array(n), H, W]
    if fused:
        assert xd == BF16 and compute == BF16
        ws = encoder_bwd_fused_workspace(n, H, W, device, ws_tag or "enc_bwd_fused")
        if ws is None:
            raise L.TacorlHipError(f"encoder_bwd_fused: geometry {H}x{W} / {len(imgs)} problems not supported")
        call("tacorl_encoder_bwd_fused", *args, int(accumulate), ptr(ws), ws.numel(), stream())
        return
    nb = L.lib().tacorl_encoder_bwd_ws_bytes(len(imgs), int_array(n), H, W)
    ws = workspace(nb, device, ws_tag or "enc_bwd")
    call("tacorl_encoder_bwd", *args, xd, compute, int(accumulate), ptr(ws), ws.numel(), stream())


# ------------------------------------------------------------------------------- MLP
def mlp_lean_ok(n, dims, ldx, ldo, ldd, compute):
    """Forward, input-gradient chain and weight gradients of this MLP site all run as the fused launches: the forward
    may then skip the hidden layers' outputs (mlp_fwd / mlp_bwd_fused_wgrad lean=True on BOTH)."""
    return compute == BF16 and bool(L.lib().tacorl_mlp_lean_supported(n, len(dims) - 1, int_array(dims), ldx, ldo, ldd))


def mlp_fwd(xs, ldx, params, acts_buf, M, dims, acts, compute=F32, params_bf16=None, lean=False):
    """params_bf16: bf16 copies of the parameter blocks -> the whole MLP runs as one launch when the
    shapes qualify (bf16 mode only); otherwise one GEMM launch per layer.
    lean: do not save hidden-layer outputs whose pre-activation is saved (see mlp_lean_ok)."""
    if (params_bf16 is not None and compute == BF16
            and L.lib().tacorl_mlp_fwd_fused_supported(len(xs), len(dims) - 1, int_array(dims), ldx)):
        call("tacorl_mlp_fwd_fused", len(xs), ptr_array(xs), ldx, ptr_array(params), ptr_array(params_bf16),
             ptr_array(acts_buf), int_array(M), len(dims) - 1, int_array(dims), int_array(acts), int(lean), stream())
        return
    assert not lean, "lean activations need the fused forward"
    call("tacorl_mlp_fwd", len(xs), ptr_array(xs), ldx, ptr_array(params), ptr_array(acts_buf), int_array(M),
         len(dims) - 1, int_array(dims), int_array(acts), compute, stream())


def mlp_fwd_gather_ok(M, dims, acts, ldx, compute, lean):
    return compute == BF16 and bool(L.lib().tacorl_mlp_fwd_fused_gather_supported(
        len(M), int_array(M), len(dims) - 1, int_array(dims), int_array(acts), ldx, int(lean)))


def mlp_fwd_gather(segs, x_out, ldx, params, params_bf16, acts_buf, M, dims, acts, lean=False, xb_out=None):
    """The fused forward with gathered layer-0 inputs.  segs[p] = [(tensor, float offset, ld, first column, row modulo)],
    <= 4 per problem, in column order; x_out[p]: tensor that also receives the assembled fp32 rows, or None.
    xb_out[p]: address (mlp_bwd_fused_xb) that also receives the rows as the weight gradients' bf16 operand, or None."""
    n = len(segs)
    sp, sl, sc, sm = [0] * (4 * n), [0] * (4 * n), [0] * (4 * n), [0] * (4 * n)
    for p, ss in enumerate(segs):
        assert 1 <= len(ss) <= 4
        for t, (ten, off, ld, c0, mod) in enumerate(ss):
            sp[4 * p + t], sl[4 * p + t], sc[4 * p + t], sm[4 * p + t] = ten.data_ptr() + 4 * off, ld, c0, mod
    xb = () if xb_out is None else (ptr_array(xb_out),)
    call("tacorl_mlp_fwd_fused_gather" + ("_xb" if xb else ""), n, int_array([len(ss) for ss in segs]),
         (C.c_void_p * (4 * n))(*[v or None for v in sp]), int_array(sl), int_array(sc), int_array(sm), ptr_array(x_out), *xb, ldx,
         ptr_array(params), ptr_array(params_bf16), ptr_array(acts_buf), int_array(M), len(dims) - 1, int_array(dims),
         int_array(acts), int(lean), stream())


def mlp_bwd(xs, ldx, params, acts_buf, d_outs, ldo, grads, d_xs, ldd, M, dims, acts, compute=F32, accumulate=False,
            ws_tag="mlp_bwd"):
    """ws_tag: scratch buffer name - calls that may overlap on different streams need different tags."""
    nb = L.lib().tacorl_mlp_bwd_ws_bytes(len(xs), int_array(M), len(dims) - 1, int_array(dims))
    ws = workspace(nb, acts_buf[0].device, ws_tag)
    call("tacorl_mlp_bwd", len(xs), ptr_array(xs), ldx, ptr_array(params), ptr_array(acts_buf), ptr_array(d_outs), ldo,
         ptr_array(grads), ptr_array(d_xs) if d_xs is not None else None, ldd, int_array(M), len(dims) - 1,
         int_array(dims), int_array(acts), compute, int(accumulate), ptr(ws), ws.numel(), stream())


def mlp_bwd_fused_ok(n, dims, ldo, ldd, compute):
    return compute == BF16 and bool(L.lib().tacorl_mlp_bwd_fused_supported(n, len(dims) - 1, int_array(dims), ldo, ldd))


def mlp_bwd_fused_pack(params, M, dims, ws_tag, device):
    """Weight transposes for mlp_bwd_fused_dgrad(prepacked=True) with the same (M, dims, ws_tag)."""
    nb = L.lib().tacorl_mlp_bwd_fused_ws_bytes(len(params), int_array(M), len(dims) - 1, int_array(dims))
    ws = workspace(nb, device, ws_tag)
    call("tacorl_mlp_bwd_fused_pack", len(params), ptr_array(params), int_array(M), len(dims) - 1, int_array(dims), ptr(ws),
         ws.numel(), stream())


def mlp_bwd_fused_xb(M, dims, ws_tag, device):
    """Per problem of the backward site (M, dims, ws_tag): the address inside its workspace where mlp_bwd_fused_wgrad reads
    layer 0's bf16 input rows - what mlp_fwd_gather(xb_out=...) may write for it (then: xb_current=True) -, or None for a
    problem that has no such region."""
    n, Ma, da = len(M), int_array(M), int_array(dims)
    ws = workspace(L.lib().tacorl_mlp_bwd_fused_ws_bytes(n, Ma, len(dims) - 1, da), device, ws_tag)
    offs = [L.lib().tacorl_mlp_bwd_fused_xb_offset(n, Ma, len(dims) - 1, da, p) for p in range(n)]
    return [None if o < 0 else ws.data_ptr() + o for o in offs]


def mlp_bwd_fused_dgrad(params, acts_buf, d_outs, ldo, d_xs, ldd, M, dims, acts, ws_tag, prepacked=False, lean=False):
    """Input-gradient chain of the whole MLP in one launch; leaves every layer's dZ in workspace(ws_tag)
    for mlp_bwd_fused_wgrad (same ws_tag, same shapes, same `lean` as the forward and the weight gradients: at
    >= 16 384 rows a lean site hands dZ over as bf16 for the LDS-DMA weight-gradient kernel)."""
    nb = L.lib().tacorl_mlp_bwd_fused_ws_bytes(len(params), int_array(M), len(dims) - 1, int_array(dims))
    ws = workspace(nb, acts_buf[0].device, ws_tag)
    call("tacorl_mlp_bwd_fused_dgrad", len(params), ptr_array(params), ptr_array(acts_buf), ptr_array(d_outs), ldo,
         ptr_array(d_xs) if d_xs is not None else ptr_array([None] * len(params)), ldd, int_array(M), len(dims) - 1,
         int_array(dims), int_array(acts), int(bool(prepacked)) | (2 if lean else 0), ptr(ws), ws.numel(), stream())


def mlp_bwd_fused_wgrad(xs, ldx, acts_buf, d_outs, ldo, grads, M, dims, acts, ws_tag, accumulate=False, lean=False,
                        xb_current=False):
    """xb_current: the site's forward has written the many-row problems' bf16 input rows (mlp_bwd_fused_xb)."""
    nb = L.lib().tacorl_mlp_bwd_fused_ws_bytes(len(xs), int_array(M), len(dims) - 1, int_array(dims))
    ws = workspace(nb, acts_buf[0].device, ws_tag)
    call("tacorl_mlp_bwd_fused_wgrad", len(xs), ptr_array(xs), ldx, ptr_array(acts_buf), ptr_array(d_outs), ldo,
         ptr_array(grads), int_array(M), len(dims) - 1, int_array(dims), int_array(acts), int(accumulate),
         int(bool(lean)) | (2 if xb_current else 0), ptr(ws), ws.numel(), stream())


def mlp_backward(tags, xs, ldx, params, acts_buf, d_outs, ldo, grads, d_xs, ldd, M, dims, acts, compute, prepacked=False,
                 lean=False, xb_current=False):
    """MLP backward.  bf16 mode: the input-gradient chain as ONE launch, the weight gradients as one launch in line
    behind it (on side streams of their own - only Adam needs them - a third set of concurrent launches beside the
    action-decoder branch's chip-wide GEMMs cost the chain more than their kernels' time: 0.8801 -> 0.8682 ms in line,
    round 3).  Otherwise: the per-layer path.  tags = (per-layer, fused) scratch buffer names; prepacked / lean: see
    mlp_bwd_fused_pack / mlp_lean_ok; xb_current: see mlp_bwd_fused_wgrad."""
    if not mlp_bwd_fused_ok(len(xs), dims, ldo, ldd, compute):
        assert not xb_current
        mlp_bwd(xs, ldx, params, acts_buf, d_outs, ldo, grads, d_xs, ldd, M, dims, acts, compute, ws_tag=tags[0])
        return
    mlp_bwd_fused_dgrad(params, acts_buf, d_outs, ldo, d_xs, ldd, M, dims, acts, tags[1], prepacked=prepacked, lean=lean)
    if any(g is not None for g in grads):
        mlp_bwd_fused_wgrad(xs, ldx, acts_buf, d_outs, ldo, grads, M, dims, acts, tags[1], lean=lean, xb_current=xb_current)


# --------------------------------------------------------------------- data movement
def pack_images(src, img_pitch, src_nchw, dst, n, Cc, H, W, src_offset=0):
    dd = BF16 if dst.dtype == torch.bfloat16 else F32
    call("tacorl_pack_images", C.c_void_p(src.data_ptr() + 4 * src_offset), img_pitch, int(src_nchw), ptr(dst), dd,
         n, Cc, H, W, stream())


# A pack job is (src, pitch, dst, n, index, stride, shift, jitter) - image_ingest.PackJob, which is built from this list and
# documents the fields - or a plain tuple of the leading fields.
JOB_FIELDS = ("src", "pitch", "dst", "n", "index", "stride", "shift", "jitter")
_JOB_ARRAY = {"src": C.c_void_p, "dst": C.c_void_p, "index": C.c_void_p, "pitch": C.c_long, "n": C.c_int, "stride": C.c_int}


def job_arrays(jobs, *fields):
    """One ctypes array per named field of the pack jobs: addresses, pitches and counts as they stand, the augmentation
    tables `shift` / `jitter` (device tensors or None) as their addresses."""
    col, k = dict(zip(JOB_FIELDS, zip(*jobs))), len(jobs)
    return [(_JOB_ARRAY[f] * k)(*col[f]) if f in _JOB_ARRAY else ptr_array(col[f]) for f in fields]


def pack_images_batch(jobs, dst_dtype_flag, H, W):
    """NCHW fp32 (C = 3) -> NHWC, one launch (H*W % 4 == 0, 16-byte aligned pointers, pitches % 4 == 0)."""
    call("tacorl_pack_images_batch", len(jobs), *job_arrays(jobs, "src", "pitch", "dst", "n"), dst_dtype_flag, H, W, stream())


def pack_images_u8_batch(jobs, dst_dtype_flag, H, W):
    """uint8 HWC frames -> normalised NHWC, one launch."""
    call("tacorl_pack_images_u8_batch", len(jobs), *job_arrays(jobs, "src", "pitch", "dst", "n"), dst_dtype_flag, H, W, stream())


def pack_images_u8_aug_batch(jobs, dst_dtype_flag, H, W, pad):
    """jobs: [(src, image_pitch_bytes, dst, n_images, shift int32 (n,2) or None, jitter f32 (n,8) or None)] - this entry point
    has no index: uint8 HWC frames -> RandomShiftsAug -> /255 -> ColorJitter -> Normalize -> NHWC, one launch."""
    for j in jobs:
        for t, dt in ((j[4], torch.int32), (j[5], torch.float32)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.shape[0] == j[3])
    call("tacorl_pack_images_u8_aug_batch", len(jobs), *job_arrays([tuple(j[:4]) + (None, 1) + tuple(j[4:]) for j in jobs],
                                                                   "src", "pitch", "dst", "shift", "jitter", "n"),
         dst_dtype_flag, H, W, int(pad), stream())


def pack_images_u8_resize_aug_batch(jobs, dst_dtype_flag, src_hw, H, W, pad):
    """uint8 HWC source frames of size src_hw, read in place or by index -> Resize(H, W) -> RandomShiftsAug(pad) -> /255 ->
    ColorJitter -> Normalize -> NHWC (the whole train pipeline of rl_train.yaml), one launch."""
    call("tacorl_pack_images_u8_resize_aug_gather_batch", len(jobs),
         *job_arrays(jobs, "src", "pitch", "index", "stride", "dst", "shift", "jitter", "n"), dst_dtype_flag, int(src_hw[0]),
         int(src_hw[1]), H, W, int(pad), stream())


def pack_images_u8_gather_batch(jobs, dst_dtype_flag, H, W):
    """image i = dataset frame index[i * stride], normalised on the way into the NHWC image buffers - the replay gather and
    the pack in one pass."""
    call("tacorl_pack_images_u8_gather_batch", len(jobs), *job_arrays(jobs, "src", "pitch", "index", "stride", "dst", "n"),
         dst_dtype_flag, H, W, stream())


def gather_frames_u8(frames, index, out):
    """out[i] = frames[index[i]] (uint8 frames resident in HBM, device int64 index)."""
    fb = frames[0].numel()
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and index.dtype == torch.int64 and index.is_cuda
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == index.numel() * fb
    call("tacorl_gather_frames_u8", ptr(frames), fb, ptr(index), ptr(out), index.numel(), stream())
    return out


def resize_frames_u8(src, out, src_pitch=None):
    """out[i] = Resize(out's H x W)(src[i]), rounded to nearest even and clamped: uint8 (n,Hs,Ws,3) -> uint8 (n,H,W,3) on the
    device (tacorl_resize_frames_u8; the sampling rule of the augmenting pack's Resize stage).  src_pitch: (bytes between
    source frames, Hs, Ws) where src is a flat uint8 buffer that holds them further apart than a frame."""
    if src_pitch is not None:
        pitch, Hs, Ws = (int(v) for v in src_pitch)
    else:
        assert src.dim() == 4 and src.shape[3] == 3 and src.shape[0] >= out.shape[0]
        Hs, Ws = int(src.shape[1]), int(src.shape[2])
        pitch = Hs * Ws * 3
    assert src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous()
    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.dim() == 4 and out.shape[3] == 3
    n, H, W = (int(v) for v in out.shape[:3])
    assert src.numel() >= (n - 1) * pitch + Hs * Ws * 3
    call("tacorl_resize_frames_u8", ptr(src), pitch, ptr(out), H * W * 3, n, Hs, Ws, H, W, stream())
    return out


# ---- the samplers over resident tables (data/resident.py).  What their four wrappers check alike:
def _all_dev(dtype, *ts):
    """Every tensor is of `dtype`, on the device and contiguous."""
    for t in ts:
        if not (t.dtype == dtype and t.is_cuda and t.is_contiguous()):
            return False
    return True


def _sampler_checks(tables, draws, B, tabs, i64, f64, status):
    """Of a sampler call: the int64 tables `tabs`, the int64 and float64 draws (B each), the action table and the int32
    status word.  (Plain loops: this runs once per batch on the trainer's thread.)"""
    for k in tabs:
        assert _all_dev(torch.int64, tables[k]), k
    for k in i64:
        assert _all_dev(torch.int64, draws[k]) and draws[k].numel() == B, k
    for k in f64:
        assert _all_dev(torch.float64, draws[k]) and draws[k].numel() == B, k
    assert tables["ep_start"].numel() == tables["ep_end"].numel() and tables["actions"].shape[0] >= tables["n_frames"]
    assert "nn_ptr" not in tables or tables["nn_ptr"].numel() == tables["n_nn"] + 1
    _f32(tables["actions"])
    assert status.dtype == torch.int32 and status.is_cuda and status.numel() == 1


def _episode_args(tables, items):
    """The leading arguments of every sampler: the item table and its length, the episode bounds and their number."""
    return ptr(tables[items]), tables[items].numel(), ptr(tables["ep_start"]), ptr(tables["ep_end"]), tables["ep_start"].numel()


def sample_transitions(tables, draws, current_horizon, ids, action, reward, done, status):
    """The transition sampler over resident tables (data/replay.py HbmTransitionReplay): tables = device tensors
    `steps`, `ep_start`, `ep_end`, `nn_ptr`, `nn_val` (int64), `actions` (N, A) f32 and the int `n_nn`, `n_frames`;
    draws = device `idx`, `strategy`, `disp` (int64) and `u_choice` (f64), B each.  Writes ids (3, B) int64
    [step | step+1 | goal], action (B, A), reward (B), done (B) f32 and raises the int32 `status` word on a clamped id."""
    B, A = ids.shape[1], tables["actions"].shape[1]
    _sampler_checks(tables, draws, B, ("steps", "ep_start", "ep_end", "nn_ptr", "nn_val"), ("idx", "strategy", "disp"),
                    ("u_choice",), status)
    assert _all_dev(torch.int64, ids) and ids.shape == (3, B)
    assert _f32(action).numel() == B * A and _f32(reward).numel() == B and _f32(done).numel() == B
    call("tacorl_sample_transitions", *_episode_args(tables, "steps"), ptr(tables["nn_ptr"]), tables["n_nn"], ptr(tables["nn_val"]),
         ptr(tables["actions"]), ptr(draws["idx"]), ptr(draws["strategy"]), ptr(draws["disp"]), ptr(draws["u_choice"]),
         int(current_horizon), int(tables["n_frames"]), B, A, ptr(ids), ptr(action), ptr(reward), ptr(done), ptr(status), stream())


def sample_relay(tables, draws, low_window, high_window, ids, action, status):
    """The relay sampler over resident tables (data/relay_replay.py HbmRelayReplay): tables = device tensors `lookup`,
    `ep_start`, `ep_end` (int64), `actions` (N, A) f32 and the int `n_frames`; draws = device `idx` (int64), `u_low`,
    `u_high` (f64), B each.  Writes ids (4, B) int64 [obs | low_level_goal | high_level_goal | high_level_action] and
    action (B, A) f32, and raises the int32 `status` word on a clamped id."""
    B, A = ids.shape[1], tables["actions"].shape[1]
    _sampler_checks(tables, draws, B, ("lookup", "ep_start", "ep_end"), ("idx",), ("u_low", "u_high"), status)
    assert _all_dev(torch.int64, ids) and ids.shape == (4, B) and _f32(action).numel() == B * A
    call("tacorl_sample_relay", *_episode_args(tables, "lookup"), ptr(tables["actions"]), int(tables["n_frames"]),
         ptr(draws["idx"]), ptr(draws["u_low"]), ptr(draws["u_high"]), int(low_window), int(high_window), B, A, ptr(ids),
         ptr(action), ptr(status), stream())


def sample_d4rl_windows(tables, draws, Tmax, G, min_window, threshold, obs, act, status, goal=None, reached=None, done=None,
                        window_size=None, ids=None):
    """The D4RL window sampler over resident tables (data/d4rl_replay.py HbmD4RLReplay): tables = device tensors `lookup`,
    `ep_start`, `ep_end` (int64), `observations` (N, S), `actions` (N, A) f32 and the int `n_frames`; draws = device `idx`,
    `window`, `disp` (int64), B each.  Writes obs (B, Tmax, S), act (B, Tmax, A) and, where given, goal (B, G), reached (B),
    done (B) f32, window_size (B) and ids (2, B) int64 = [start | goal_step]; raises the int32 `status` word on a clamp."""
    B = draws["idx"].numel()
    S, A = tables["observations"].shape[1], tables["actions"].shape[1]
    _sampler_checks(tables, draws, B, ("lookup", "ep_start", "ep_end"), ("idx", "window", "disp"), (), status)
    assert _f32(tables["observations"]).shape[0] >= tables["n_frames"]
    for t, n in ((obs, B * Tmax * S), (act, B * Tmax * A), (goal, B * G), (reached, B), (done, B)):
        assert t is None or _f32(t).numel() == n, (None if t is None else tuple(t.shape), n)
    for t, n in ((window_size, B), (ids, 2 * B)):
        assert t is None or (_all_dev(torch.int64, t) and t.numel() == n)
    call("tacorl_sample_d4rl_windows", *_episode_args(tables, "lookup"), ptr(tables["observations"]), ptr(tables["actions"]),
         int(tables["n_frames"]), ptr(draws["idx"]), ptr(draws["window"]), ptr(draws["disp"]), B, int(Tmax), S, A, int(G),
         int(min_window), float(threshold), ptr(obs), ptr(act), ptr(goal), ptr(reached), ptr(done), ptr(window_size), ptr(ids),
         ptr(status), stream())


def sample_play_windows(tables, draws, Tmax, min_window, ids, act, disp_out, window_size, status, goal_augmentation=False):
    """The play-window sampler over resident tables (data/play_replay.py HbmPlayReplay): tables = device tensors `lookup`,
    `ep_start`, `ep_end`, `nn_ptr`, `nn_val` (int64), `actions` (N, A) f32 and the ints `n_nn`, `n_frames`, `last_end`;
    draws = device `idx`, `window_size`, `strategy`, `disp`, `noise_step` (int64; read with goal_augmentation only) and
    `u_choice`, `u_random_state` (f64), B each.  Writes ids (B * Tmax + B) int64 = [window frames (b, t) | goal], act
    (B, Tmax, A) f32, disp_out (B) and window_size (B) int64; raises the int32 `status` word on a clamp."""
    B, A = draws["idx"].numel(), tables["actions"].shape[1]
    ints = ("idx", "window_size", "strategy", "disp") + (("noise_step",) if goal_augmentation else ())
    _sampler_checks(tables, draws, B, ("lookup", "ep_start", "ep_end", "nn_ptr", "nn_val"), ints, ("u_choice", "u_random_state"),
                    status)
    assert _all_dev(torch.int64, ids, disp_out, window_size)
    assert ids.numel() == B * Tmax + B and disp_out.numel() == B and window_size.numel() == B
    assert _f32(act).numel() == B * Tmax * A
    n_nn = int(tables["n_nn"])
    call("tacorl_sample_play_windows", *_episode_args(tables, "lookup"), ptr(tables["nn_ptr"]) if n_nn else None, n_nn,
         ptr(tables["nn_val"]) if n_nn else None, ptr(tables["actions"]), int(tables["n_frames"]), int(tables["last_end"]),
         ptr(draws["idx"]), ptr(draws["window_size"]), ptr(draws["strategy"]), ptr(draws["disp"]),
         ptr(draws["noise_step"]) if goal_augmentation else None, ptr(draws["u_choice"]), ptr(draws["u_random_state"]), B,
         int(Tmax), A, int(min_window), ptr(ids), ptr(act), ptr(disp_out), ptr(window_size), ptr(status), stream())


# The blocking of the k-NN search kernel (knn_ops.hip; tacorl_knn_l2_tile / tacorl_knn_l2_query_block answer the same, which
# tests/test_nn_table_cpu.py checks): database rows per LDS tile, queries per workgroup for k <= 32 and for k <= 64.
KNN_TILE, KNN_QUERY_BLOCK, KNN_QUERY_BLOCK_K64 = 128, 256, 128
KNN_MAX_D, KNN_MAX_K = 32, 64


def knn_l2_supported(D, k):
    return bool(L.lib().tacorl_knn_l2_supported(int(D), int(k)))


def knn_l2(points, k, q0=0, n_queries=None, nbr_row=None, nbr_dist=None, want_dist=True):
    """Exact L2 k-NN of the rows [q0, q0 + n_queries) of `points` against all its rows, by the definition of
    include/tacorl_hip.h tacorl_knn_l2 (fp32 direct form, (distance, row) order).  points: (N, D) fp32 device tensor whose
    rows are dense (stride(1) == 1; a column slice of a wider table is fine).  Returns nbr_row (n_queries, k) int32 and
    nbr_dist (n_queries, k) fp32 (None with want_dist=False)."""
    assert points.dim() == 2 and points.dtype == torch.float32 and points.is_cuda, (points.dtype, points.device, points.dim())
    N, D = points.shape
    assert N >= 1 and (N == 1 or points.stride(0) >= D) and (D == 1 or points.stride(1) == 1), (points.shape, points.stride())
    ld = int(points.stride(0)) if N > 1 else D
    n_queries = N - q0 if n_queries is None else int(n_queries)
    if not knn_l2_supported(D, k):
        raise L.TacorlHipError(f"knn_l2: D = {D} (1..{KNN_MAX_D}) / k = {k} (1..{KNN_MAX_K}) not supported")
    if nbr_row is None:
        nbr_row = torch.empty(n_queries, k, dtype=torch.int32, device=points.device)
    if nbr_dist is None and want_dist:
        nbr_dist = torch.empty(n_queries, k, dtype=torch.float32, device=points.device)
    for t, dt in ((nbr_row, torch.int32), (nbr_dist, torch.float32)):
        assert t is None or (t.dtype == dt and t.is_cuda and t.is_contiguous() and t.numel() == n_queries * k)
    call("tacorl_knn_l2", ptr(points), N, D, ld, int(q0), n_queries, int(k), ptr(nbr_row), ptr(nbr_dist), stream())
    return nbr_row, nbr_dist


def nn_margin_filter(nbr_row, step_of_row, margin, q0=0, nn_steps=None, count=None):
    """The reference's temporal filter behind the top-k (tacorl_nn_margin_filter): nbr_row (n_queries, k) int32 rows of the
    queries [q0, q0 + n_queries), step_of_row (N) int64.  Returns nn_steps (n_queries, k) int64 - the surviving steps packed
    left in list order, -1 after - and count (n_queries) int32."""
    assert nbr_row.dim() == 2 and nbr_row.dtype == torch.int32 and nbr_row.is_cuda and nbr_row.is_contiguous()
    assert step_of_row.dim() == 1 and step_of_row.dtype == torch.int64 and step_of_row.is_cuda and step_of_row.is_contiguous()
    nq, k = nbr_row.shape
    if nn_steps is None:
        nn_steps = torch.empty(nq, k, dtype=torch.int64, device=nbr_row.device)
    if count is None:
        count = torch.empty(nq, dtype=torch.int32, device=nbr_row.device)
    assert nn_steps.dtype == torch.int64 and nn_steps.is_cuda and nn_steps.is_contiguous() and nn_steps.numel() == nq * k
    assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.numel() == nq
    call("tacorl_nn_margin_filter", ptr(nbr_row), nq, k, int(q0), ptr(step_of_row), step_of_row.numel(), int(margin),
         ptr(nn_steps), ptr(count), stream())
    return nn_steps, count


# ---- exact t-SNE (tsne_ops.hip; definition: include/tacorl_hip.h)
TSNE_MAX_N, TSNE_MAX_D = 8192, 32


def tsne_supported(N, D):
    return bool(L.lib().tacorl_tsne_supported(int(N), int(D)))


def tsne_workspace(N, device):
    """A fresh workspace for the three t-SNE calls on an (N, .) table (uint8), or TacorlHipError."""
    nbytes = int(L.lib().tacorl_tsne_workspace_bytes(int(N)))
    if nbytes == 0:
        raise L.TacorlHipError(f"tsne: N = {N} not supported (4..{TSNE_MAX_N})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def tsne_workspace_views(ws, N):
    """{xn (N, 32), attr (N, 2), rep (N, 2), zrow (N)}: float views of what the last tsne_affinities / tsne_step left in ws."""
    off = (C.c_long * 4)()
    call("tacorl_tsne_workspace_offsets", int(N), off)
    f = ws.view(torch.float32)
    return {k: f[o // 4: o // 4 + N * w].view(N, w) if w > 1 else f[o // 4: o // 4 + N]
            for k, o, w in zip(("xn", "attr", "rep", "zrow"), off, (32, 2, 2, 1))}


def _tsne_ws(ws, N):
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.is_contiguous(), (ws.dtype, ws.device)
    return ptr(ws), ws.numel()


def tsne_affinities(X, perplexity, P=None, beta=None, status=None, ws=None):
    """The symmetric affinity matrix of exact t-SNE.  X: (N, D) fp32 device tensor with dense rows (a column slice of a wider
    table is fine).  Returns P (N, N) fp32, beta (N) fp32, status (2) int32 ([rows whose search hit the step cap, all-equal
    table]) and the workspace; nothing is read back here."""
    assert X.dim() == 2 and X.dtype == torch.float32 and X.is_cuda, (X.dtype, X.device, X.dim())
    N, D = X.shape
    assert N >= 1 and (N == 1 or X.stride(0) >= D) and (D == 1 or X.stride(1) == 1), (X.shape, X.stride())
    ld = int(X.stride(0)) if N > 1 else D
    if not tsne_supported(N, D):
        raise L.TacorlHipError(f"tsne_affinities: N = {N} (4..{TSNE_MAX_N}) / D = {D} (1..{TSNE_MAX_D}) not supported")
    dev = X.device
    P = torch.empty(N, N, device=dev) if P is None else P
    beta = torch.empty(N, device=dev) if beta is None else beta
    status = torch.empty(2, dtype=torch.int32, device=dev) if status is None else status
    ws = tsne_workspace(N, dev) if ws is None else ws
    assert P.dtype == torch.float32 and P.is_cuda and P.is_contiguous() and P.numel() == N * N
    assert beta.dtype == torch.float32 and beta.is_cuda and beta.is_contiguous() and beta.numel() == N
    assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() == 2
    call("tacorl_tsne_affinities", ptr(X), N, D, ld, float(perplexity), ptr(P), ptr(beta), ptr(status), *_tsne_ws(ws, N), stream())
    return P, beta, status, ws


def _tsne_state(N, *ts):
    for t in ts:
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == 2 * N, (t.dtype, t.device, t.shape)


def tsne_step(P, Y, u, gains, exaggeration, momentum, lr, ws):
    """One t-SNE iteration in place on Y, u, gains (each (N, 2) fp32); attr, rep and Z_i stay in ws (tsne_workspace_views)."""
    assert P.dim() == 2 and P.shape[0] == P.shape[1] and P.dtype == torch.float32 and P.is_cuda and P.is_contiguous()
    N = P.shape[0]
    _tsne_state(N, Y, u, gains)
    call("tacorl_tsne_step", ptr(P), N, ptr(Y), ptr(u), ptr(gains), float(exaggeration), float(momentum), float(lr),
         *_tsne_ws(ws, N), stream())


def tsne_kl(P, Y, ws, out=None):
    """KL(P || Q(Y)) as a (1,) fp32 device tensor."""
    assert P.dim() == 2 and P.shape[0] == P.shape[1] and P.dtype == torch.float32 and P.is_cuda and P.is_contiguous()
    N = P.shape[0]
    _tsne_state(N, Y)
    out = torch.empty(1, device=P.device) if out is None else out
    assert out.dtype == torch.float32 and out.is_cuda and out.numel() == 1
    call("tacorl_tsne_kl", ptr(P), ptr(Y), N, ptr(out), *_tsne_ws(ws, N), stream())
    return out


# ---- neighbour-sparse t-SNE (tsne_ops.hip; definition: include/tacorl_hip.h)
TSNE_NBR_MAX_N, TSNE_NBR_MAX_K = 131072, 192


def tsne_nbr_k(perplexity):
    """K = floor(3 perplexity), the product taken in fp32 as the library takes it."""
    import numpy as np

    return int(np.floor(np.float32(3.0) * np.float32(perplexity)))


def tsne_nbr_supported(N, D, K):
    return bool(L.lib().tacorl_tsne_nbr_supported(int(N), int(D), int(K)))


def tsne_nbr_workspace(N, device):
    """A fresh workspace for the neighbour-sparse t-SNE calls on an (N, .) table (uint8), or TacorlHipError."""
    nbytes = int(L.lib().tacorl_tsne_nbr_workspace_bytes(int(N)))
    if nbytes == 0:
        raise L.TacorlHipError(f"tsne_nbr: N = {N} not supported (4..{TSNE_NBR_MAX_N})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def tsne_nbr_workspace_views(ws, N):
    """{xn (N, 32), attr (N, 2), rep (N, 2), zrow (N)}: float views of what the last tsne_nbr_affinities / tsne_nbr_step left."""
    off = (C.c_long * 4)()
    call("tacorl_tsne_nbr_workspace_offsets", int(N), off)
    f = ws.view(torch.float32)
    return {k: f[o // 4: o // 4 + N * w].view(N, w) if w > 1 else f[o // 4: o // 4 + N]
            for k, o, w in zip(("xn", "attr", "rep", "zrow"), off, (32, 2, 2, 1))}


def _dense_rows(X):
    assert X.dim() == 2 and X.dtype == torch.float32 and X.is_cuda, (X.dtype, X.device, X.dim())
    N, D = X.shape
    assert N >= 1 and (N == 1 or X.stride(0) >= D) and (D == 1 or X.stride(1) == 1), (X.shape, X.stride())
    return N, D, int(X.stride(0)) if N > 1 else D


def tsne_nbr_knn(points, K):
    """The K nearest other rows of every row of points (N, D), by the definition of include/tacorl_hip.h "neighbour-sparse
    t-SNE": nbr_row (N, K) int32, nbr_dist (N, K) fp32."""
    N, D, ld = _dense_rows(points)
    if not tsne_nbr_supported(N, D, K):
        raise L.TacorlHipError(f"tsne_nbr_knn: N = {N} (4..{TSNE_NBR_MAX_N}) / D = {D} (1..{TSNE_MAX_D}) / K = {K} "
                               f"(1..min({TSNE_NBR_MAX_K}, N - 1)) not supported")
    nbr_row = torch.empty(N, K, dtype=torch.int32, device=points.device)
    nbr_dist = torch.empty(N, K, dtype=torch.float32, device=points.device)
    call("tacorl_tsne_nbr_knn", ptr(points), N, D, ld, int(K), ptr(nbr_row), ptr(nbr_dist), stream())
    return nbr_row, nbr_dist


def tsne_nbr_affinities(X, perplexity, ws=None):
    """The neighbour-sparse symmetric P.  X: (N, D) fp32 device tensor with dense rows.  Returns a dict: nbr_row, nbr_dist and
    cond (N, K), beta (N), the CSR row_ptr (N + 1) int32 / col / val (capacity 2 N K; row_ptr[N] entries are in use),
    status (2) int32 and ws; nothing is read back here."""
    N, D, ld = _dense_rows(X)
    K = tsne_nbr_k(perplexity) if perplexity >= 1.0 else 0
    if not tsne_nbr_supported(N, D, K):
        raise L.TacorlHipError(f"tsne_nbr_affinities: N = {N} (4..{TSNE_NBR_MAX_N}) / D = {D} (1..{TSNE_MAX_D}) / perplexity = "
                               f"{perplexity} (K = floor(3 perplexity) in 3..min({TSNE_NBR_MAX_K}, N - 1)) not supported")
    dev = X.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(nbr_row=torch.empty(N, K, **i32), nbr_dist=torch.empty(N, K, device=dev), cond=torch.empty(N, K, device=dev),
               beta=torch.empty(N, device=dev), row_ptr=torch.empty(N + 1, **i32), col=torch.empty(2 * N * K, **i32),
               val=torch.empty(2 * N * K, device=dev), status=torch.empty(2, **i32),
               ws=tsne_nbr_workspace(N, dev) if ws is None else ws)
    call("tacorl_tsne_nbr_affinities", ptr(X), N, D, ld, float(perplexity), ptr(out["nbr_row"]), ptr(out["nbr_dist"]),
         ptr(out["cond"]), ptr(out["beta"]), ptr(out["row_ptr"]), ptr(out["col"]), ptr(out["val"]), 2 * N * K, ptr(out["status"]),
         *_tsne_ws(out["ws"], N), stream())
    return out


def _tsne_csr(row_ptr, col, val):
    assert row_ptr.dtype == torch.int32 and row_ptr.is_cuda and row_ptr.is_contiguous() and row_ptr.dim() == 1
    assert col.dtype == torch.int32 and col.is_cuda and col.is_contiguous() and val.dtype == torch.float32 and val.is_cuda
    assert val.is_contiguous() and col.numel() == val.numel()
    return row_ptr.numel() - 1


def tsne_nbr_step(row_ptr, col, val, Y, u, gains, exaggeration, momentum, lr, ws):
    """One neighbour-sparse t-SNE iteration in place on Y, u, gains (each (N, 2) fp32); attr, rep and Z_i stay in ws."""
    N = _tsne_csr(row_ptr, col, val)
    _tsne_state(N, Y, u, gains)
    call("tacorl_tsne_nbr_step", ptr(row_ptr), ptr(col), ptr(val), N, ptr(Y), ptr(u), ptr(gains), float(exaggeration),
         float(momentum), float(lr), *_tsne_ws(ws, N), stream())


def tsne_nbr_kl(row_ptr, col, val, Y, ws, out=None):
    """KL(P || Q(Y)) over the stored entries as a (1,) fp32 device tensor."""
    N = _tsne_csr(row_ptr, col, val)
    _tsne_state(N, Y)
    out = torch.empty(1, device=Y.device) if out is None else out
    assert out.dtype == torch.float32 and out.is_cuda and out.numel() == 1
    call("tacorl_tsne_nbr_kl", ptr(row_ptr), ptr(col), ptr(val), ptr(Y), N, ptr(out), *_tsne_ws(ws, N), stream())
    return out


def _at(t, off):
    return C.c_void_p(t.data_ptr() + 4 * off)


# ---- tracing aid: device time marks between the launches of a step (off unless trace_marks() is called)
_marks = None


def trace_marks(device, slots=64):
    """Switch time marks on: every mark(name) call appends one 1-thread launch that stores the device clock.
    Returns a reader: reader() -> [(name, microseconds since the first mark)] of the last run / graph replay."""
    global _marks
    import torch

    buf = torch.zeros(slots, dtype=torch.int64, device=device)
    _marks = {"buf": buf, "names": []}

    def reader():
        t = buf.cpu().tolist()
        names = _marks["names"]
        t0 = min(t[: len(names)]) if names else 0
        return sorted(((n, (t[i] - t0) / 100.0) for i, n in enumerate(names)), key=lambda r: r[1])

    return reader


def mark(name):
    if _marks is None:
        return
    names = _marks["names"]
    if name not in names:
        names.append(name)
    call("tacorl_time_mark", ptr(_marks["buf"]), names.index(name), stream())


class prep_batch:
    """`with ops.prep_batch():` - the weight-only preparation launches issued inside (to_bf16 mirrors, the MLP backward
    sites' transposed weights, the encoders' FC-tail transposes) become ONE launch at the end of the block, on the
    stream current THERE (tacorl_prep_batch_begin / _end).  enabled = False: every launch on its own (the tests' comparator)."""
    enabled = True

    def __enter__(self):
        self.on = prep_batch.enabled
        if self.on:
            call("tacorl_prep_batch_begin")
        return self

    def __exit__(self, et, ev, tb):
        if self.on:
            rc = L.lib().tacorl_prep_batch_end(stream())
            if et is None and rc != 0:
                raise RuntimeError(f"tacorl_prep_batch_end failed ({rc})")
        return False


class reduce_batch:
    """`with ops.reduce_batch():` - the slab reduces of the one-launch MLP weight gradients issued inside are summed by ONE
    launch at the end of the block (on the stream current there); the gradients are complete only after it.
    Off unless the caller asks (auto) or a test sets enabled: it measured slower on the headline step (same-process A/B:
    0.8201 -> 0.8276 ms/step) - the five reduces run in launch gaps of the step's other branch where they stand; as one
    launch at the end of the backward they are 10 us of their own in front of the optimiser."""
    enabled = False

    def __init__(self, auto=False):
        """auto: the caller's own judgement for this block (the actor-critic engine: many-row Q problems, where the reduces
        are large enough for one launch to win - C5 1.597 -> 1.586 ms/step)."""
        self.auto = bool(auto)

    def __enter__(self):
        self.on = reduce_batch.enabled or self.auto
        if self.on:
            call("tacorl_reduce_batch_begin")
        return self

    def __exit__(self, et, ev, tb):
        if self.on:
            rc = L.lib().tacorl_reduce_batch_end(stream())
            if et is None and rc != 0:
                raise RuntimeError(f"tacorl_reduce_batch_end failed ({rc})")
        return False


_copy_batch = None


class copy_batch:
    """`with ops.copy_batch():` turns the copy_cols calls inside into ONE launch (<= 32 per launch).
    The copies of a batch must be independent: none may read what another one writes."""

    def __enter__(self):
        global _copy_batch
        assert _copy_batch is None, "copy_batch does not nest"
        _copy_batch = []
        return self

    def __exit__(self, et, ev, tb):
        global _copy_batch
        items, _copy_batch = _copy_batch, None
        if et is not None:
            return False
        for i in range(0, len(items), 32):
            ch = items[i:i + 32]
            cols = list(zip(*ch))
            call("tacorl_copy_cols_batch", len(ch), (C.c_void_p * len(ch))(*cols[0]), int_array(cols[1]),
                 (C.c_void_p * len(ch))(*cols[2]), int_array(cols[3]), int_array(cols[4]), int_array(cols[5]),
                 int_array(cols[6]), int_array(cols[7]), stream())
        return False


def copy_cols(src, src_off, ld_src, dst, dst_off, ld_dst, rows, cols, src_row_mod=0, accumulate=False):
    if _copy_batch is not None:
        _copy_batch.append((src.data_ptr() + 4 * src_off, ld_src, dst.data_ptr() + 4 * dst_off, ld_dst, rows, cols,
                            src_row_mod, int(accumulate)))
        return
    call("tacorl_copy_cols", _at(src, src_off), ld_src, _at(dst, dst_off), ld_dst, rows, cols, src_row_mod,
         int(accumulate), stream())


def reduce_rows_mod(src, src_off, ld_in, dst, dst_off, ld_out, B, cols, reps):
    call("tacorl_reduce_rows_mod", _at(src, src_off), ld_in, _at(dst, dst_off), ld_out, B, cols, reps, stream())


def uniform_actions(u01, dst, dst_off, ld_dst, rows, A, discrete_gripper):
    call("tacorl_uniform_actions", ptr(u01), _at(dst, dst_off), ld_dst, rows, A, int(discrete_gripper), stream())


def tanh_normal_sample(head, ld_head, eps, gumbel_u, hard, act_out, act_off, ld_act, logp, grip_idx, n, M, Ac):
    call("tacorl_tanh_normal_sample", ptr(head), ld_head, ptr(eps), ptr(gumbel_u), int(hard), _at(act_out, act_off),
         ld_act, ptr(logp), ptr(grip_idx), n, M, Ac, stream())


def cem_supported(N, A, E, hidden, q_layers, compute):
    return bool(L.lib().tacorl_cem_supported(int(N), int(A), int(E), int(hidden), int(q_layers), int(compute)))


def cem_refine(s, params, params_bf16, mean0, eps, out, N, A, E, hidden, q_layers, iters, n_elite, min_std, max_std, alpha,
               discrete_gripper, compute, trace=None):
    """One launch: the whole CEM refinement of out.shape[0] problem rows.  s / params / params_bf16: per net (1 = that net's
    Q, 2 = the twin minimum); trace: None or (population, Q, elite indices int32, mean, std) tensors to fill."""
    R = out.shape[0]
    nb = L.lib().tacorl_cem_ws_bytes(R, N, A, E, hidden, q_layers, compute)
    ws = workspace(nb, out.device, "cem")
    call("tacorl_cem_refine", R, len(s), ptr_array([_f32(t) for t in s]), ptr_array(params),
         ptr_array(params_bf16) if params_bf16 is not None else None, ptr(mean0), ptr(_f32(eps)), ptr(_f32(out)), N, A, E,
         hidden, q_layers, iters, n_elite, float(min_std), float(max_std), float(alpha), int(bool(discrete_gripper)), compute,
         *([ptr(t) for t in trace] if trace is not None else [None] * 5), ptr(ws), ws.numel(), stream())


def adam_step_batch(items, mirrors=None):
    """items: list of (param, grad, m, v, lr, max_norm, step_counter, target_or_None, tau) - one
    norm (+ step counter) launch and one update launch for all of them.
    mirrors: optional list of (bf16 mirror of param or None, bf16 mirror of target or None), written by the update launch."""
    k = len(items)
    nb = L.lib().tacorl_adam_batch_ws_bytes(k)
    ws = workspace(nb, items[0][0].device, "adam_batch")
    mir = ptr_array([m_[0] for m_ in mirrors]) if mirrors else None
    tmir = ptr_array([m_[1] for m_ in mirrors]) if mirrors else None
    call("tacorl_adam_step_batch_mirror", k, ptr_array([i[0] for i in items]), ptr_array([i[1] for i in items]),
         ptr_array([i[2] for i in items]), ptr_array([i[3] for i in items]), (C.c_long * k)(*[i[0].numel() for i in items]),
         (C.c_float * k)(*[float(i[4]) for i in items]), (C.c_float * k)(*[float(i[5]) for i in items]),
         ptr_array([i[6] for i in items]), ptr_array([i[7] for i in items]), (C.c_float * k)(*[float(i[8]) for i in items]),
         mir, tmir, ptr(ws), ws.numel(), stream())
    touched(*[i[0] for i in items], *[i[7] for i in items if i[7] is not None])


def touched(*tensors):
    """The library's kernels write parameter blocks through raw pointers, which torch's version counters do not see;
    bump them by hand (host-side, no launch) so that caches keyed on `tensor._version` - the frozen-network weight
    preparation - also notice optimiser steps.  Views share their base's counter."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


def adam_step(param, grad, m, v, lr, max_norm, step_counter, target=None, tau=0.0):
    n = param.numel()
    nb = L.lib().tacorl_adam_ws_bytes(n)
    ws = workspace(nb, param.device, "adam")
    call("tacorl_adam_step", ptr(param), ptr(grad), ptr(m), ptr(v), n, float(lr), float(max_norm), ptr(step_counter),
         ptr(target), float(tau), ptr(ws), ws.numel(), stream())
    touched(param, *([target] if target is not None else []))
