"""Kernel-level tests of the small kernels in front of every training step: the fp32 image packs (tacorl_pack_images,
tacorl_pack_images_batch / _window_batch), the uint8 packs and the frame gather (tacorl_pack_images_u8_batch /
_u8_gather_batch, tacorl_gather_frames_u8) and the row assembly (tacorl_copy_cols / _batch, tacorl_birnn_swap_rows,
tacorl_reduce_rows_mod, tacorl_stage_transition).

The packs are moves plus one cast: the reference is torch's own permute / indexing / .to(torch.bfloat16) and every
comparison is of bit patterns (so -0.0 is not +0.0).  The uint8 packs are compared with ((x / 255 - 0.5) / 0.5).to(dt)
evaluated on the CPU - where a case is too large to copy, through the 256-entry table of that expression.  Copies are
exact against torch indexing, accumulating copies against one fp32 add; the row reduction is compared with the fp64 sum
under test_heads_gpu's rule and bitwise with the wave-order sum.

Outputs are pre-filled with NaN (uint8: 249, integers: -7), have leading dimensions wider than their rows where the
ABI has them and a guard tail behind every written range.  One case per kernel lies past the kernel's block cap, where
its grid-stride loop runs; those are generated and referenced on the device.  Refusal checks pass only what the
launchers reject before launching anything.

(The uint8 packs take H W 3 % 16 == 0, so their smallest frame is 48 bytes, 2 x 8 pixels; 16 bytes is the smallest
frame of tacorl_gather_frames_u8.)"""
import ctypes as C

import pytest
import torch

from tests.test_heads_gpu import EINVAL, NAN, _check, _dev, _rc, _untouched

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
U8_SENTINEL = 249
DTYPES = [(F32, torch.float32), (BF16, torch.bfloat16)]
# bf16 round-to-nearest-even ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), their neighbours, signed zero, +-1
SPECIAL = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, 1.0, -1.0, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,
           1 + 2.0 ** -8 - 2.0 ** -20, 0.0, -(1 + 3 * 2.0 ** -8)]


def _ops():
    from tacorl_amd import ops

    return ops


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _exact(name, got, ref):
    """Bit-exact comparison where the tensors live (the large cases stay on the device)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = _bits(got) != _bits(ref.to(got.device))
    nbad = int(bad.sum())
    print(f"bit-exact {name}: {bad.numel()} elements")
    if nbad:
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {nbad} of {bad.numel()} differ, first at {first}: "
                             f"{got[tuple(first)].item()} vs {ref[tuple(first)].item()}")


def _fill(shape, dt, dev):
    if dt == torch.uint8:
        return torch.full(shape, U8_SENTINEL, dtype=dt, device=dev)
    return torch.full(shape, NAN, dtype=dt, device=dev)


def _untouched_u8(name, t):
    assert (t == U8_SENTINEL).all(), f"{name}: padding / guard elements were written"


def _longs(vals):
    return (C.c_long * len(vals))(*[int(v) for v in vals])


def _images(n, pitch, used, seed):
    """n fp32 images at a pitch of `pitch` floats (`used` of them the image), the special values at both ends."""
    x = torch.randn(n, pitch, generator=torch.Generator().manual_seed(seed))
    k = min(len(SPECIAL), used)
    x[0, :k] = torch.tensor(SPECIAL[:k])
    x[n - 1, used - k:used] = torch.tensor(SPECIAL[:k])
    return x


# ============================================================================ fp32 packs
def test_pack_images_layouts():
    """NCHW / NHWC sources, C in {1, 3, 4}, both destination dtypes, H W = 35 (no multiple of 4), a pitch wider than
    the image and a source offset."""
    ops = _ops()
    dev = _dev()
    n, H, W, off = 3, 5, 7, 3
    for nchw in (1, 0):
        for Cc in (1, 3, 4):
            used = Cc * H * W
            pitch = used + 5
            x = _images(n, pitch, used, seed=10 * Cc + nchw)
            img = x[:, :used].reshape(n, Cc, H, W).permute(0, 2, 3, 1) if nchw else x[:, :used].reshape(n, H, W, Cc)
            back = torch.cat([torch.full((off,), NAN), x.flatten()]).to(dev)
            for flag, dt in DTYPES:
                dst = _fill((n * used + 8,), dt, dev)
                ops.call("tacorl_pack_images", ops.ptr(back[off:]), pitch, nchw, ops.ptr(dst), flag, n, Cc, H, W, ops.stream())
                torch.cuda.synchronize()
                tag = f"pack_images nchw={nchw} C={Cc} {dt}"
                _exact(tag, dst[:n * used].cpu().view(n, H, W, Cc), img.contiguous().to(dt))
                _untouched(f"{tag} guard", dst[n * used:])


def test_pack_images_past_block_cap():
    """5 x 459 x 461 = 1 057 995 pixels > 4096 x 256: the grid-stride loop runs."""
    ops = _ops()
    dev = _dev()
    n, Cc, H, W = 5, 3, 459, 461
    torch.manual_seed(3)
    x = torch.randn(n, Cc, H, W, device=dev)
    dst = _fill((n * Cc * H * W + 8,), torch.bfloat16, dev)
    ops.call("tacorl_pack_images", ops.ptr(x), Cc * H * W, 1, ops.ptr(dst), BF16, n, Cc, H, W, ops.stream())
    torch.cuda.synchronize()
    _exact("pack_images past the block cap", dst[:-8].view(n, H, W, Cc), x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16))
    _untouched("pack_images past the block cap: guard", dst[-8:])


def _window_call(jobs, flag, H, W, njobs=None, first_array=True, last_array=True):
    """jobs: dicts with src, pitch, dst, n, first, last, T.  The raw return code."""
    ops = _ops()
    col = lambda k: [j[k] for j in jobs]  # noqa: E731
    return _rc("tacorl_pack_images_window_batch", len(jobs) if njobs is None else njobs, ops.ptr_array(col("src")),
               _longs(col("pitch")), ops.ptr_array(col("dst")), ops.int_array(col("n")),
               ops.ptr_array(col("first")) if first_array else None, ops.ptr_array(col("last")) if last_array else None,
               ops.int_array(col("T")), flag, H, W, ops.stream())


# (images, window T or 0, kind): eight jobs, a zero-count job in the middle and a window job behind it
WINDOW_JOBS = [(3, 0, "plain"), (6, 2, "window"), (1, 0, "plain"), (0, 0, "empty"), (9, 3, "window"), (3, 0, "strided"),
               (7, 0, "padded"), (4, 2, "window")]


@pytest.mark.parametrize("flag,dt", DTYPES)
def test_pack_images_window_batch(flag, dt):
    """Eight jobs of different counts in one launch.  A window job writes image b T to dst_first[b] and image b T + T - 1
    to dst_last[b] besides its own destination; the launcher drops the zero-count job and must keep every job's window,
    dst_first and dst_last with it."""
    dev = _dev()
    H, W = 6, 10
    used = 3 * H * W
    jobs = []
    for ji, (n, T, kind) in enumerate(WINDOW_JOBS):
        pitch = used + 8 if kind == "padded" else used
        if kind == "strided":  # the first frames of the T = 3 window job's source: a pitch of T images
            src_h, src_d, pitch = jobs[4]["host"], jobs[4]["src"], 3 * used
            img = src_h[::3, :used]
        else:
            src_h = _images(max(n, 1), pitch, used, seed=40 + ji)
            src_d = src_h.to(dev)
            img = src_h[:n, :used]
        nb = n // T if T else 0
        j = dict(src=src_d, pitch=pitch, n=n, T=T, host=src_h, kind=kind,
                 ref=img.reshape(n, 3, H, W).permute(0, 2, 3, 1).contiguous().to(dt),
                 dst=_fill((max(n, 1) * used + 16,), dt, dev),
                 first=_fill((nb * used + 16,), dt, dev) if T else None,
                 last=_fill((nb * used + 16,), dt, dev) if T else None)
        jobs.append(j)
    assert _window_call(jobs, flag, H, W) == 0
    torch.cuda.synchronize()
    for ji, j in enumerate(jobs):
        tag = f"window_batch {dt} job{ji} ({j['kind']})"
        n, T = j["n"], j["T"]
        if n == 0:
            _untouched(f"{tag}: the zero-count job's destination", j["dst"])
            continue
        _exact(tag, j["dst"][:n * used].cpu().view(n, H, W, 3), j["ref"])
        _untouched(f"{tag} guard", j["dst"][n * used:])
        if T:
            nb = n // T
            w = j["ref"].view(nb, T, H, W, 3)
            _exact(f"{tag} dst_first", j["first"][:nb * used].cpu().view(nb, H, W, 3), w[:, 0].contiguous())
            _exact(f"{tag} dst_last", j["last"][:nb * used].cpu().view(nb, H, W, 3), w[:, T - 1].contiguous())
            _untouched(f"{tag} dst_first guard", j["first"][nb * used:])
            _untouched(f"{tag} dst_last guard", j["last"][nb * used:])
    # the plain entry point: the same jobs without windows
    plain = [dict(j, dst=_fill((max(j["n"], 1) * used + 16,), dt, dev)) for j in jobs]
    ops = _ops()
    col = lambda k: [j[k] for j in plain]  # noqa: E731
    ops.call("tacorl_pack_images_batch", len(plain), ops.ptr_array(col("src")), _longs(col("pitch")), ops.ptr_array(col("dst")),
             ops.int_array(col("n")), flag, H, W, ops.stream())
    torch.cuda.synchronize()
    for ji, j in enumerate(plain):
        n = j["n"]
        if n:
            _exact(f"pack_images_batch {dt} job{ji}", j["dst"][:n * used].cpu().view(n, H, W, 3), j["ref"])
        _untouched(f"pack_images_batch {dt} job{ji} guard", j["dst"][n * used:])


def test_pack_images_window_batch_past_block_cap():
    """513 x 128 x 128 = 8 404 992 pixels in the window job (T = 3): 8208 workgroups' worth of pixel quads > 8192."""
    dev = _dev()
    H, W, n, T = 128, 128, 513, 3
    used = 3 * H * W
    torch.manual_seed(5)
    big, small = torch.randn(n, 3, H, W, device=dev), torch.randn(2, 3, H, W, device=dev)
    nb = n // T
    dt = torch.bfloat16
    jobs = [dict(src=small, pitch=used, n=2, T=0, dst=_fill((2 * used + 16,), dt, dev), first=None, last=None),
            dict(src=big, pitch=used, n=n, T=T, dst=_fill((n * used + 16,), dt, dev),
                 first=_fill((nb * used + 16,), dt, dev), last=_fill((nb * used + 16,), dt, dev))]
    assert _window_call(jobs, BF16, H, W) == 0
    torch.cuda.synchronize()
    ref = big.permute(0, 2, 3, 1).contiguous().to(dt)
    _exact("window job past the block cap", jobs[1]["dst"][:n * used].view(n, H, W, 3), ref)
    w = ref.view(nb, T, H, W, 3)
    _exact("window job past the block cap: dst_first", jobs[1]["first"][:nb * used].view(nb, H, W, 3), w[:, 0].contiguous())
    _exact("window job past the block cap: dst_last", jobs[1]["last"][:nb * used].view(nb, H, W, 3), w[:, T - 1].contiguous())
    _exact("small job beside it", jobs[0]["dst"][:2 * used].view(2, H, W, 3), small.permute(0, 2, 3, 1).contiguous().to(dt))
    for name, t, k in (("dst", jobs[1]["dst"], n), ("dst_first", jobs[1]["first"], nb), ("dst_last", jobs[1]["last"], nb),
                       ("small dst", jobs[0]["dst"], 2)):
        _untouched(f"past the block cap: {name} guard", t[k * used:])


def test_pack_images_window_batch_refuses():
    """Everything here is rejected by the launcher's argument checks, which all run before the launch."""
    dev = _dev()
    H, W = 6, 10
    used = 3 * H * W
    src = torch.zeros(6 * used + 8, device=dev)
    mk = lambda **kw: dict(dict(src=src, pitch=used, n=6, T=0, dst=_fill((6 * used + 8,), torch.float32, dev), first=None,  # noqa: E731
                                last=None), **kw)
    aux = [_fill((3 * used,), torch.float32, dev) for _ in range(2)]
    win = mk(T=2, first=aux[0], last=aux[1])
    bad = {
        "9 jobs": ([mk() for _ in range(9)], {}),
        "0 jobs": ([mk()], dict(njobs=0)),
        "a source misaligned by 4 bytes": ([mk(src=src[1:])], {}),
        "a destination misaligned by 4 bytes": ([mk(dst=_fill((6 * used + 8,), torch.float32, dev)[1:])], {}),
        "pitch % 4 != 0": ([mk(pitch=used + 2)], {}),
        "window 1": ([dict(win, T=1)], {}),
        "n_img % T != 0": ([dict(win, T=4)], {}),
        "a window job whose dst_last entry is NULL": ([dict(win, last=None)], {}),
        "a window job without a dst_last array": ([win], dict(last_array=False)),
        "a window job whose dst_first is misaligned": ([dict(win, first=aux[0][1:])], {}),
    }
    outs = []
    for name, (jobs, kw) in bad.items():
        assert _window_call(jobs, F32, H, W, **kw) == EINVAL, name
        outs += [j["dst"] for j in jobs] + [j[k] for j in jobs for k in ("first", "last") if j[k] is not None]
    assert _window_call([mk()], F32, 5, 7) == EINVAL, "H W % 4 != 0"
    torch.cuda.synchronize()
    for t in outs:
        _untouched("refused call: destination", t)
    assert _window_call([win], F32, H, W) == 0  # the same window job, well-formed
    torch.cuda.synchronize()
    assert (win["dst"][:6 * used] == 0).all() and (aux[0] == 0).all() and (aux[1] == 0).all()


# ============================================================================ uint8 packs and gather
def _norm(x, dt):
    """ToTensor and Normalize(0.5, 0.5) in fp32, then the cast - test_pack_images_u8's reference."""
    return ((x.float().div(255) - 0.5) / 0.5).to(dt)


def _u8_call(jobs, flag, H, W, stride_array=True, gather=True):
    """jobs: dicts with src, pitch (bytes), idx (device int64 or None), stride, dst, n."""
    ops = _ops()
    col = lambda k: [j[k] for j in jobs]  # noqa: E731
    if not gather:
        return _rc("tacorl_pack_images_u8_batch", len(jobs), ops.ptr_array(col("src")), _longs(col("pitch")),
                   ops.ptr_array(col("dst")), ops.int_array(col("n")), flag, H, W, ops.stream())
    return _rc("tacorl_pack_images_u8_gather_batch", len(jobs), ops.ptr_array(col("src")), _longs(col("pitch")),
               ops.ptr_array(col("idx")), ops.int_array(col("stride")) if stride_array else None, ops.ptr_array(col("dst")),
               ops.int_array(col("n")), flag, H, W, ops.stream())


def _u8_jobs(frames, frames_d, specs, dt, dev):
    """specs: (kind, ids or None, stride, n, pitch in frames).  Every id lies inside the dataset."""
    fb = frames[0].numel()
    jobs = []
    for kind, ids, stride, n, pf in specs:
        if ids is not None:
            assert 0 <= min(ids) and max(ids) < frames.shape[0] and len(ids) >= (n - 1) * stride + 1
            picked = [ids[i * stride] for i in range(n)]
        else:
            picked = [i * pf for i in range(n)]
            assert not picked or picked[-1] < frames.shape[0]
        jobs.append(dict(kind=kind, src=frames_d, pitch=fb * pf, stride=stride, n=n,
                         idx=torch.tensor(ids, dtype=torch.int64, device=dev) if ids is not None else None,
                         dst=_fill((max(n, 1) * fb + 16,), dt, dev),
                         ref=_norm(frames[picked], dt) if n else None))
    return jobs


def _u8_verify(tag, jobs, frames):
    fb = frames[0].numel()
    for ji, j in enumerate(jobs):
        n = j["n"]
        if n:
            _exact(f"{tag} job{ji} ({j['kind']})", j["dst"][:n * fb].cpu().view(j["ref"].shape), j["ref"])
        _untouched(f"{tag} job{ji} guard", j["dst"][n * fb:])


@pytest.mark.parametrize("flag,dt", DTYPES)
def test_pack_images_u8_all_bytes_and_index_tables(flag, dt):
    """The smallest frame (2 x 8 pixels, three 16-byte chunks); 256 frames built so that every byte value appears at every
    one of the 16 byte positions of a chunk.  Jobs in one launch: no index (a NULL entry) beside index tables of stride 1
    and T, descending and repeated ids, a zero-count job in the middle, a strided plain job."""
    dev = _dev()
    H, W, T = 2, 8, 4
    f, p = torch.arange(256).view(256, 1), torch.arange(48).view(1, 48)
    frames = ((f + 17 * p + 5 * (p // 16)) % 256).to(torch.uint8).view(256, H, W, 3)
    for pos in range(16):
        assert len(set(frames.view(256, 48)[:, pos].tolist())) == 256
    frames_d = frames.to(dev)
    g = torch.Generator().manual_seed(9)
    table = torch.randint(0, 256, (64 * T,), generator=g).tolist()
    table[4], table[8] = table[0], table[0]  # the same frame three times in the strided picks
    specs = [("no index", None, 1, 256, 1), ("descending ids", list(range(255, -1, -1)), 1, 256, 1),
             ("id table at stride T", table, T, 64, 1), ("zero count", None, 1, 0, 1),
             ("repeated ids", [5, 5, 5, 9, 9, 0, 255, 255], 1, 8, 1), ("every T-th frame by pitch", None, 1, 64, T),
             ("id table at stride 1", table, 1, 64 * T, 1)]
    jobs = _u8_jobs(frames, frames_d, specs, dt, dev)
    assert _u8_call(jobs, flag, H, W) == 0
    torch.cuda.synchronize()
    _u8_verify(f"u8_gather_batch {dt}", jobs, frames)
    # the plain entry point (no index at all) over the jobs that have none
    plain = _u8_jobs(frames, frames_d, [s for s in specs if s[1] is None], dt, dev)
    assert _u8_call(plain, flag, H, W, gather=False) == 0
    torch.cuda.synchronize()
    _u8_verify(f"u8_batch {dt}", plain, frames)


def test_pack_images_u8_real_frame_and_null_stride_array():
    """84 x 84 frames; index tables with the stride array NULL (stride 1)."""
    dev = _dev()
    H, W = 84, 84
    frames = torch.randint(0, 256, (12, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    frames_d = frames.to(dev)
    specs = [("reversed ids", list(range(11, -1, -1)), 1, 12, 1), ("no index", None, 1, 12, 1),
             ("repeated ids", [3, 3, 11, 0, 3], 1, 5, 1)]
    for flag, dt in DTYPES:
        jobs = _u8_jobs(frames, frames_d, specs, dt, dev)
        assert _u8_call(jobs, flag, H, W, stride_array=False) == 0
        torch.cuda.synchronize()
        _u8_verify(f"u8_gather_batch 84x84 {dt}", jobs, frames)


def test_pack_images_u8_gather_past_block_cap():
    """1600 gathered 84 x 84 frames = 2 116 800 chunks of 16 bytes > 8192 x 256."""
    dev = _dev()
    H, W, n, nf = 84, 84, 1600, 64
    fb = H * W * 3
    torch.manual_seed(6)
    frames_d = torch.randint(0, 256, (nf, H, W, 3), dtype=torch.uint8, device=dev)
    idx = torch.randint(0, nf, (n,), device=dev)
    dt = torch.bfloat16
    lut = _norm(torch.arange(256, dtype=torch.uint8), dt).to(dev)  # the reference expression, evaluated on the CPU
    job = dict(src=frames_d, pitch=fb, idx=idx, stride=1, n=n, dst=_fill((n * fb + 16,), dt, dev))
    assert _u8_call([job], BF16, H, W) == 0
    torch.cuda.synchronize()
    _exact("u8 gather past the block cap", job["dst"][:n * fb].view(n, H, W, 3), lut[frames_d[idx].int()])
    _untouched("u8 gather past the block cap: guard", job["dst"][n * fb:])


def _gather(frames_d, fb, idx, dst, n):
    ops = _ops()
    return _rc("tacorl_gather_frames_u8", ops.ptr(frames_d), fb, ops.ptr(idx), ops.ptr(dst), n, ops.stream())


def test_gather_frames_u8():
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    for fb, nf in ((16, 40), (84 * 84 * 3, 9)):
        frames = torch.randint(0, 256, (nf, fb), dtype=torch.uint8, generator=g)
        frames_d = frames.to(dev)
        ids = list(range(nf - 1, -1, -1)) + [2, 2, 2, 0, nf - 1, nf - 1]  # reversed, then repeated
        idx = torch.tensor(ids, dtype=torch.int64, device=dev)
        n = len(ids)
        dst = _fill((n * fb + 32,), torch.uint8, dev)
        assert _gather(frames_d, fb, idx, dst, n) == 0
        torch.cuda.synchronize()
        _exact(f"gather_frames_u8 frame_bytes={fb}", dst[:n * fb].cpu().view(n, fb), frames[ids])
        _untouched_u8(f"gather_frames_u8 frame_bytes={fb} guard", dst[n * fb:])
        none = _fill((n * fb,), torch.uint8, dev)
        assert _gather(frames_d, fb, idx, none, 0) == 0  # n = 0 writes nothing
        torch.cuda.synchronize()
        _untouched_u8("gather_frames_u8 n = 0", none)
    # refusals: all checked before the launch
    dst = _fill((2 * fb,), torch.uint8, dev)
    assert _gather(frames_d, 24, idx, dst, 1) == EINVAL  # frame_bytes % 16
    assert _gather(frames_d.view(-1)[4:], fb, idx, dst, 1) == EINVAL  # a misaligned base
    assert _gather(frames_d, fb, idx, dst[4:], 1) == EINVAL  # a misaligned destination
    assert _gather(frames_d, fb, None, dst, 1) == EINVAL  # NULL index
    torch.cuda.synchronize()
    _untouched_u8("refused gathers", dst)


def test_gather_frames_u8_past_block_cap():
    """3200 frames of 84 x 84 x 3 bytes = 4 233 600 chunks > 16384 x 256."""
    dev = _dev()
    fb, nf, n = 84 * 84 * 3, 48, 3200
    torch.manual_seed(7)
    frames_d = torch.randint(0, 256, (nf, fb), dtype=torch.uint8, device=dev)
    idx = torch.randint(0, nf, (n,), device=dev)
    dst = _fill((n * fb + 32,), torch.uint8, dev)
    assert _gather(frames_d, fb, idx, dst, n) == 0
    torch.cuda.synchronize()
    _exact("gather_frames_u8 past the block cap", dst[:n * fb].view(n, fb), frames_d[idx])
    _untouched_u8("gather_frames_u8 past the block cap: guard", dst[n * fb:])


# ============================================================================ row assembly
def _copy_case(rows, cols, mod, acc, dev, seed):
    """A copy descriptor with pre-offset pointers: the source is the window [1:, 2:2+cols] of a backing array that has
    `rows` + 2 rows whatever `mod` is (rows beyond the ones a wrapped copy reads hold other values), the destination the
    window [1:1+rows, 3:3+cols] of a NaN-filled one."""
    g = torch.Generator().manual_seed(seed)
    ld_src, ld_dst = cols + 3, cols + 5
    sb = torch.randn(rows + 2, ld_src, generator=g)
    db = torch.full((rows + 3, ld_dst), NAN)
    d0 = torch.randn(rows, cols, generator=g)
    if acc:
        db[1:1 + rows, 3:3 + cols] = d0
    r = torch.arange(rows)
    ref = sb[1:, 2:2 + cols][r % mod if mod > 0 else r]
    if acc:
        ref = d0 + ref  # one fp32 add
    sb_d, db_d = sb.to(dev), db.to(dev)
    return dict(sb=sb_d, db=db_d, src=sb_d[1:, 2:], dst=db_d[1:, 3:], ld_src=ld_src, ld_dst=ld_dst, rows=rows, cols=cols,
                mod=mod, acc=acc, ref=ref)


def _copy_verify(tag, c):
    got = c["db"].cpu()
    rows, cols = c["rows"], c["cols"]
    mask = torch.zeros_like(got, dtype=torch.bool)
    mask[1:1 + rows, 3:3 + cols] = True
    if rows:
        _exact(tag, got[1:1 + rows, 3:3 + cols], c["ref"])
    _untouched(f"{tag}: columns beyond cols, rows beyond rows", got[~mask])


def test_copy_cols():
    """dst[r][0:cols] (+)= src[r % src_row_mod][0:cols]: expand_obs on embeddings and the accumulating copies."""
    ops = _ops()
    dev = _dev()
    B, seed = 5, 0
    for rows in (15, 13):  # a multiple of B and not
        for mod in (0, B):
            for cols in (1, 7, 64):
                for acc in (0, 1):
                    seed += 1
                    c = _copy_case(rows, cols, mod, acc, dev, seed)
                    ops.call("tacorl_copy_cols", ops.ptr(c["src"]), c["ld_src"], ops.ptr(c["dst"]), c["ld_dst"], rows, cols, mod,
                             acc, ops.stream())
                    torch.cuda.synchronize()
                    _copy_verify(f"copy_cols rows={rows} cols={cols} mod={mod} acc={acc}", c)


def _copy_big(rows, cols, mod, dev):
    """An accumulating wrapped copy generated and referenced on the device (an element visited twice would show)."""
    ld_src, ld_dst = cols + 3, cols + 5
    sb = torch.randn(rows + 2, ld_src, device=dev)
    db = torch.full((rows + 3, ld_dst), NAN, device=dev)
    d0 = torch.randn(rows, cols, device=dev)
    db[1:1 + rows, 3:3 + cols] = d0
    ref = d0 + sb[1:, 2:2 + cols][torch.arange(rows, device=dev) % mod]
    return dict(sb=sb, db=db, src=sb[1:, 2:], dst=db[1:, 3:], ld_src=ld_src, ld_dst=ld_dst, rows=rows, cols=cols, mod=mod,
                acc=1, ref=ref)


def _copy_big_verify(tag, c):
    rows, cols = c["rows"], c["cols"]
    _exact(tag, c["db"][1:1 + rows, 3:3 + cols], c["ref"])
    mask = torch.zeros_like(c["db"], dtype=torch.bool)
    mask[1:1 + rows, 3:3 + cols] = True
    _untouched(f"{tag}: outside the window", c["db"][~mask])


def test_copy_cols_past_block_cap():
    """8200 x 64 = 524 800 elements > 2048 x 256."""
    ops = _ops()
    dev = _dev()
    torch.manual_seed(11)
    c = _copy_big(8200, 64, 1025, dev)
    ops.call("tacorl_copy_cols", ops.ptr(c["src"]), c["ld_src"], ops.ptr(c["dst"]), c["ld_dst"], c["rows"], c["cols"], c["mod"], 1,
             ops.stream())
    torch.cuda.synchronize()
    _copy_big_verify("copy_cols past the block cap", c)


def _copy_batch(cs, n=None, arrays=True):
    ops = _ops()
    col = lambda k: [c[k] for c in cs]  # noqa: E731
    return _rc("tacorl_copy_cols_batch", len(cs) if n is None else n, ops.ptr_array(col("src")), ops.int_array(col("ld_src")),
               ops.ptr_array(col("dst")), ops.int_array(col("ld_dst")), ops.int_array(col("rows")), ops.int_array(col("cols")),
               ops.int_array(col("mod")) if arrays else None, ops.int_array(col("acc")) if arrays else None, ops.stream())


@pytest.mark.parametrize("arrays", [True, False])
def test_copy_cols_batch_32_descriptors(arrays):
    """32 descriptors of different shapes, a zero-row one in the middle (the launcher compacts the table), src_row_mod and
    accumulate once as arrays and once NULL (plain copies)."""
    dev = _dev()
    B = 5
    cs = []
    for i in range(32):
        rows = 0 if i == 15 else (15, 13, 5, 1)[i % 4]
        cols = (1, 7, 64)[i % 3]
        mod, acc = (B if i % 2 else 0, (i // 2) % 2) if arrays else (0, 0)
        cs.append(_copy_case(rows, cols, mod, acc, dev, seed=100 + i))
    assert _copy_batch(cs, arrays=arrays) == 0
    torch.cuda.synchronize()
    for i, c in enumerate(cs):
        _copy_verify(f"copy_cols_batch arrays={arrays} descriptor {i}", c)


def test_copy_cols_batch_past_block_cap_and_refusal():
    """2051 x 64 = 131 264 elements in the largest descriptor > 512 x 256; 33 descriptors are refused."""
    dev = _dev()
    torch.manual_seed(12)
    big = _copy_big(2051, 64, 293, dev)
    small = _copy_case(13, 7, 5, 1, dev, seed=77)
    assert _copy_batch([small, big]) == 0
    torch.cuda.synchronize()
    _copy_big_verify("copy_cols_batch past the block cap", big)
    _copy_verify("copy_cols_batch: the small descriptor beside it", small)
    cs = [_copy_case(3, 7, 0, 0, dev, seed=200)] * 33
    assert _copy_batch(cs) == EINVAL
    torch.cuda.synchronize()
    _untouched("33 descriptors: destination", cs[0]["db"])


SWAP_CASES = [(1, 5, 3), (5, 1, 3), (7, 16, 33), (64, 129, 64)]  # the last: 528 384 elements > 2048 x 256


@pytest.mark.parametrize("no,ni,cols", SWAP_CASES)
def test_birnn_swap_rows(no, ni, cols):
    """dst[i n_outer + o] = src[o n_inner + i]; applied again with the roles swapped it returns the input."""
    ops = _ops()
    dev = _dev()
    ld_src, ld_dst = cols + 2, cols + 3
    torch.manual_seed(no * ni)
    src = torch.randn(no * ni, ld_src, device=dev)
    dst, back = _fill((no * ni + 1, ld_dst), torch.float32, dev), _fill((no * ni + 1, ld_src), torch.float32, dev)
    ops.call("tacorl_birnn_swap_rows", ops.ptr(src), ld_src, ops.ptr(dst), ld_dst, no, ni, cols, ops.stream())
    ops.call("tacorl_birnn_swap_rows", ops.ptr(dst), ld_dst, ops.ptr(back), ld_src, ni, no, cols, ops.stream())
    torch.cuda.synchronize()
    ref = src.view(no, ni, ld_src)[:, :, :cols].permute(1, 0, 2).reshape(ni * no, cols)
    _exact(f"birnn_swap_rows {no}x{ni}x{cols}", dst[:no * ni, :cols], ref)
    _exact(f"birnn_swap_rows {no}x{ni}x{cols} twice", back[:no * ni, :cols], src[:, :cols])
    for name, t in (("dst", dst), ("back", back)):
        _untouched(f"birnn_swap_rows {name}: padding columns", t[:no * ni, cols:])
        _untouched(f"birnn_swap_rows {name}: guard row", t[no * ni:])


def test_birnn_swap_rows_refuses():
    ops = _ops()
    dev = _dev()
    src, dst = torch.zeros(35, 5, device=dev), _fill((35, 5), torch.float32, dev)
    run = lambda ls, ld, no, ni, cols: _rc("tacorl_birnn_swap_rows", ops.ptr(src), ls, ops.ptr(dst), ld, no, ni, cols,  # noqa: E731
                                           ops.stream())
    assert run(4, 5, 7, 5, 5) == EINVAL and run(5, 4, 7, 5, 5) == EINVAL  # ld < cols
    assert run(5, 5, 0, 5, 5) == EINVAL and run(5, 5, 7, 0, 5) == EINVAL and run(5, 5, 7, 5, 0) == EINVAL
    torch.cuda.synchronize()
    _untouched("refused swaps", dst)


def _wave_order_sum(x, B, cols, reps):
    """The order test_reduce_rows_mod_batch spells out: wave w adds j = w, w + 4, ...; the four meet in wave order."""
    part = []
    for w in range(4):
        acc = torch.zeros(B, cols, device=x.device)
        for j in range(w, reps, 4):
            acc = acc + x[j * B:(j + 1) * B, :cols]
        part.append(acc)
    return ((part[0] + part[1]) + part[2]) + part[3]


# reps 1..3 leave three, two, one waves without a row to add; B cols = 35 and 165: no multiple of 64, one and three
# workgroups; the last case: 524 800 outputs > 8192 x 64
REDUCE_CASES = [(5, 7, r) for r in (1, 2, 3, 4, 5)] + [(33, 5, r) for r in (1, 3, 5)] + [(8200, 64, 5)]


@pytest.mark.parametrize("B,cols,reps", REDUCE_CASES)
def test_reduce_rows_mod(B, cols, reps):
    ops = _ops()
    dev = _dev()
    ld_in, ld_out = cols + 3, cols + 2
    torch.manual_seed(B + reps)
    x = torch.randn(reps * B, ld_in, device=dev)
    out = _fill((B + 1, ld_out), torch.float32, dev)
    ops.call("tacorl_reduce_rows_mod", ops.ptr(x), ld_in, ops.ptr(out), ld_out, B, cols, reps, ops.stream())
    torch.cuda.synchronize()
    tag = f"reduce_rows_mod B={B} cols={cols} reps={reps}"
    xs = x.view(reps, B, ld_in)[:, :, :cols]
    _check(f"{tag} vs fp64", out[:B, :cols], xs.double().sum(0), xs.sum(0))
    _exact(f"{tag} vs the wave-order sum", out[:B, :cols], _wave_order_sum(x, B, cols, reps))
    _untouched(f"{tag}: padding columns", out[:B, cols:])
    _untouched(f"{tag}: guard row", out[B:])


F1 = torch.tensor(1.0)
FLOAT_DISP = [torch.nextafter(F1, torch.tensor(0.0)).item(), 1.0, torch.nextafter(F1, torch.tensor(2.0)).item(), 0.0, -1.0,
              2.0, 1.0]
INT64_DISP = [2 ** 32 + 1, 1, 0, -1, 2 ** 32, 1 - 2 ** 32, 1, 3]


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("kind", ["float", "int64"])
def test_stage_transition(B, kind):
    """reward = done = float(disp == 1): the fp32 neighbours of 1 give 0, and so does the int64 2^32 + 1, whose low word
    is 1.  The action copy with n_acts = 0 (NULL pointers), 3 (< B for B = 257) and more than B; done may be NULL."""
    ops = _ops()
    dev = _dev()
    pat, code, dt = (FLOAT_DISP, 0, torch.float32) if kind == "float" else (INT64_DISP, 1, torch.int64)
    disp = torch.tensor([pat[i % len(pat)] for i in range(B)], dtype=dt)
    ref = (disp == 1).float()
    assert ref[0] == 0 and (B == 1 or ref[1] == 1)
    disp_d = disp.to(dev)
    g = torch.Generator().manual_seed(B)
    for n_acts in (0, 3, 7 * B + 2):
        for with_done in (True, False):
            acts = torch.randn(max(n_acts, 1), generator=g)
            acts_d, out = acts.to(dev), _fill((n_acts + 4,), torch.float32, dev)
            reward, done = _fill((B + 4,), torch.float32, dev), _fill((B + 4,), torch.float32, dev)
            ops.call("tacorl_stage_transition", ops.ptr(disp_d), code, ops.ptr(reward), ops.ptr(done) if with_done else None, B,
                     ops.ptr(acts_d) if n_acts else None, ops.ptr(out) if n_acts else None, n_acts, ops.stream())
            torch.cuda.synchronize()
            tag = f"stage_transition {kind} B={B} n_acts={n_acts} done={with_done}"
            _exact(f"{tag} reward", reward[:B].cpu(), ref)
            _untouched(f"{tag} reward guard", reward[B:])
            if with_done:
                _exact(f"{tag} done", done[:B].cpu(), ref)
                _untouched(f"{tag} done guard", done[B:])
            else:
                _untouched(f"{tag} done (NULL pointer given)", done)
            if n_acts:
                _exact(f"{tag} actions", out[:n_acts].cpu(), acts)
            _untouched(f"{tag} actions guard", out[n_acts:])
