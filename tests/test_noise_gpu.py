"""tacorl_noise_fill (csrc/noise_ops.hip) against the NumPy restatement (tacorl_amd.noise.philox_restatement): one launch over
nine segments at the smallest shapes that can go wrong - ragged groups (inner 7, 6, 2), both layouts, a keep mask, a segment
longer than a workgroup's span (1 025 groups) and one of a single group, with segment boundaries inside workgroups.  Uniforms
and keep masks bit for bit, normals inside tests/noise_ref.py's bound against fp64 on the same words, padding untouched, shards
bit-identical on the device, bad tables refused with nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

from tacorl_amd import noise as N
from tests import noise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (kind, draw id, B_local, inner, n_outer, outer_major[, keep_p]); groups of four: 6, 6, 12, 12, 12, 3, 384 | 1 025 | 1
# -> boundaries at 435 (inside workgroup 1) and 1 460 (inside workgroup 5)
SPECS = [("normal", 0, 3, 7, 1, False), ("normal", 1, 3, 6, 1, False), ("normal", 2, 3, 6, 2, True), ("normal", 9, 3, 16, 1, False),
         ("uniform", 4, 3, 7, 2, True), ("uniform", 5, 3, 2, 1, False), ("keep", 32, 3, 16 * 32, 1, False, 0.9),
         ("normal", 10, 1025, 3, 1, False), ("normal", 3, 1, 3, 1, False)]


def _buffers(n_f32, n_u8):
    return (torch.full((n_f32,), float("nan"), device=DEV), torch.full((max(n_u8, 1),), 0xFF, dtype=torch.uint8, device=DEV))


def _fill(tab, f32, u8, seed, step, sample0):
    N.DeviceNoise(seed, step).fill(tab, f32, u8, sample0)
    torch.cuda.synchronize()
    return f32.cpu().numpy(), u8.cpu().numpy()


def _seg_view(seg, f32, u8):
    flat = (u8 if seg.kind == N.KEEP else f32)[seg.offset: seg.offset + seg.numel]
    return flat.reshape((seg.n_outer, seg.B_local, seg.inner) if seg.outer_major else (seg.B_local, seg.n_outer, seg.inner))


@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("sample0", [0, 5])
def test_nine_segments_one_launch(sample0, step):
    seed = 0x0123_4567_89AB_CDEF
    tab, n_f32, n_u8 = R.carve(SPECS)
    assert tab.n_groups == 435 + 1025 + 1 and len(tab) == 9
    f32, u8 = _fill(tab, *_buffers(n_f32, n_u8), seed, step, sample0)
    written = {False: np.zeros(n_f32, bool), True: np.zeros(max(n_u8, 1), bool)}
    worst = 0.0
    for seg in tab.segments:
        got, want = _seg_view(seg, f32, u8), R.expected(seg, seed, step, sample0)
        written[seg.kind == N.KEEP][seg.offset: seg.offset + seg.numel] = True
        if seg.kind == N.NORMAL:
            assert np.isfinite(got).all()
            ratio = np.abs(got.astype(np.float64) - want) / R.normal_bound(want)
            worst = max(worst, float(ratio.max()))
        elif seg.kind == N.UNIFORM:
            assert (got == want.astype(np.float32)).all() and (got.astype(np.float64) == want).all()
        else:
            assert (got == want).all() and 0 < got.mean() < 1
    print(f"sample0 {sample0} step {step}: worst |z_gpu - z_fp64| / bound = {worst:.4f} (K = {R.K})")
    assert worst <= 1.0
    assert np.isnan(f32[~written[False]]).all() and (~written[False]).sum() >= 4 * 8   # padding between the buffers: untouched
    assert (u8[~written[True]] == 0xFF).all() and (~written[True]).sum() >= 4


def test_shards_are_bit_identical_on_the_device():
    """B = 8 in one fill == two B = 4 fills with sample0 0 and 4, for every kind and layout (normals too: same code, same words)."""
    seed, step = 99, 3
    shapes = [("normal", 0, 7, 1, False), ("normal", 2, 6, 4, True), ("normal", 1, 16, 2, False), ("uniform", 4, 7, 4, True),
              ("uniform", 5, 2, 1, False), ("keep", 33, 100, 1, False, 0.9)]
    spec = lambda B: [(s[0], s[1], B) + tuple(s[2:]) for s in shapes]  # noqa: E731
    tab8, nf8, nu8 = R.carve(spec(8))
    tab4, nf4, nu4 = R.carve(spec(4))
    full = _fill(tab8, *_buffers(nf8, nu8), seed, step, 0)
    lo = _fill(tab4, *_buffers(nf4, nu4), seed, step, 0)
    hi = _fill(tab4, *_buffers(nf4, nu4), seed, step, 4)
    for s8, s4 in zip(tab8.segments, tab4.segments):
        ax = 1 if s8.outer_major else 0
        joined = np.concatenate([_seg_view(s4, *lo), _seg_view(s4, *hi)], axis=ax)
        got = _seg_view(s8, *full)
        assert joined.tobytes() == got.tobytes(), s8.draw_id
        assert not np.array_equal(_seg_view(s4, *lo), _seg_view(s4, *hi))


def test_refusals_write_nothing():
    from tacorl_amd import _lib

    L = _lib.lib()
    f32, u8 = _buffers(64, 64)
    seg = lambda **kw: N.Segment(**{**dict(offset=0, kind="normal", draw_id=0, B_local=3, inner=7), **kw})  # noqa: E731
    past = N.SegmentTable([seg(), seg(offset=44)], 64, 64)           # 21 floats from 44: one past the buffer's 64
    outer = N.SegmentTable([seg()], 1 << 30, 64)
    outer.c_table.seg[0].n_outer = 65536
    kind = N.SegmentTable([seg(), seg(kind=3, offset=24)], 64, 64)
    for tab in (past, outer, kind):
        rc = L.tacorl_noise_fill(C.byref(tab.c_table), len(tab), C.c_void_p(f32.data_ptr()), C.c_void_p(u8.data_ptr()), 1, 0, 0,
                                 _lib.stream())
        assert rc < 0
    torch.cuda.synchronize()
    assert torch.isnan(f32).all() and (u8 == 0xFF).all()
    ok = N.SegmentTable([seg(), seg(offset=43)], 64, 64)             # ... and the same table one float earlier is taken
    N.DeviceNoise(1).fill(ok, f32, u8)
    torch.cuda.synchronize()
    assert torch.isfinite(f32[:21]).all() and torch.isfinite(f32[43:]).all() and torch.isnan(f32[21:43]).all()
