"""The NumPy restatement of the device-noise generator (tacorl_amd/noise.py): Philox4x32-10 known answers, shard invariance,
moments and independence over 2^20 draws, the meaning of the GPU test's fp32 bound, and the entry point's refusals (which
happen before any launch, so they run without a GPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tacorl_amd import noise as N
from tests import noise_ref as R


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, want):
    assert _hex(N.philox4x32_10(np.array(counter), np.array(key))) == want


def test_counter_layout():
    """words of (seed, step, draw, sample, group) = block(counter (q, sample0 + b, draw << 16 | k, step), key (lo, hi))."""
    seed, step, did = 0x1234_5678_9ABC_DEF0, 7, 11
    w = N.philox_words(seed, step, did, B_local=3, inner=10, n_outer=2, sample0=5)
    assert w.shape == (3, 2, 3, 4)
    one = N.philox4x32_10(np.array([2, 5 + 1, did << 16 | 1, step]), np.array([seed & 0xFFFFFFFF, seed >> 32]))
    assert (w[1, 1, 2] == one).all()
    u = N.philox_restatement(seed, step, did, "uniform", 3, 10, 2, 5, outer_major=True)
    assert u.shape == (2, 3, 10) and u[1, 1, 9] == (int(one[1]) >> 8) * 2.0 ** -24  # element 9: group 2, word 1
    assert ((u >= 0) & (u < 1)).all() and (u.astype(np.float32).astype(np.float64) == u).all()


@pytest.mark.parametrize("n_outer", [1, 4])
@pytest.mark.parametrize("inner", [7, 6, 2, 16])
@pytest.mark.parametrize("kind", ["normal", "uniform", "keep"])
def test_shard_invariance(kind, inner, n_outer):
    for om in (False, True):
        kw = dict(kind=kind, inner=inner, n_outer=n_outer, outer_major=om, keep_p=0.9)
        full = N.philox_restatement(3, 2, 4, B_local=8, **kw)
        lo, hi = N.philox_restatement(3, 2, 4, B_local=4, **kw), N.philox_restatement(3, 2, 4, B_local=4, sample0=4, **kw)
        assert (np.concatenate([lo, hi], axis=1 if om else 0) == full).all()
        assert not (lo == hi).all()


def test_ids_are_distinct_and_steps_bounded():
    ids = list(N.DRAW_IDS.values()) + [N.dropout_id(i) for i in range(N.DROPOUT_MAX)]
    assert len(set(ids)) == len(ids) and max(ids) <= 65535
    with pytest.raises(ValueError):
        N.DeviceNoise(1, step=1 << 32)
    g = N.DeviceNoise(1, step=(1 << 32) - 1)
    with pytest.raises(ValueError):
        g.advance()
    with pytest.raises(ValueError):
        N.SegmentTable([N.Segment(0, "normal", 0, 1, 4, n_outer=65536)], 1 << 20)


# ------------------------------------------------------------------------------------------------ moments
B_M, INNER_M = 4096, 256  # 2^20 draws


@functools.lru_cache(maxsize=None)
def _draws(seed, step, did, kind):
    return N.philox_restatement(seed, step, did, kind, B_M, INNER_M)


@pytest.mark.parametrize("seed", [0, 1234])
def test_moments_and_independence(seed):
    x = _draws(seed, 3, N.DRAW_IDS["eps_pi"], "normal")
    u = _draws(seed, 3, N.DRAW_IDS["u_rand"], "uniform")
    stats = {f"normal {k}": v for k, v in R.normal_stats(x).items()}
    stats.update({f"uniform {k}": v for k, v in R.uniform_stats(u).items()})
    stats["corr step+1"] = R.corr_stat(x, _draws(seed, 4, N.DRAW_IDS["eps_pi"], "normal"))
    stats["corr other draw"] = R.corr_stat(x, _draws(seed, 3, N.DRAW_IDS["eps_next"], "normal"))
    stats["corr neighbour"] = R.corr_stat(x[..., :-1], x[..., 1:])
    print({k: round(float(v), 3) for k, v in stats.items()}, "max |z|", float(np.abs(x).max()))
    bad = {k: v for k, v in stats.items() if not abs(v) <= 5.0}
    assert not bad, bad
    assert np.isfinite(x).all() and np.abs(x).max() < np.sqrt(2 * 24 * np.log(2.0)) + 1e-9  # |z| <= sqrt(-2 ln 2^-24) = 5.77


# ------------------------------------------------------------------------------------------------ the bound's meaning
def test_bound_is_the_documented_sum():
    assert R.K == 2 * (R.E_LOG / 2 + R.E_SQRT + R.E_SINCOS + 0.5)
    z = np.array([0.0, 0.5, -3.0])
    assert (R.normal_bound(z) == R.K * 2.0 ** -23 * np.array([1.0, 1.0, 3.0])).all()


@pytest.mark.parametrize("defect", ["swap", "bits23", "pairs02"])
def test_bound_tells_planted_defects_from_rounding(defect):
    """Each defect moves some normal of a 2^16-draw buffer by at least 10 x the bound the GPU test allows there (so the GPU
    test, which checks every element, fails on it) - and the restatement with no defect is the restatement."""
    w = N.philox_words(0, 0, 0, 256, 256)
    z = N.normal_from_words(w)
    assert (R.defective_normals(w, None) == z).all()
    ratio = np.abs(R.defective_normals(w, defect) - z) / R.normal_bound(z)
    print(defect, "largest change / bound", float(ratio.max()), "elements past 10 x bound", float((ratio >= 10).mean()))
    assert ratio.max() >= 10.0


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def _fill(tab, n_seg=None, f32=4096, u8=4096, sample0=0, seed=1, step=0):
    from tacorl_amd import _lib

    L = _lib.lib()
    return L.tacorl_noise_fill(C.byref(tab.c_table), len(tab) if n_seg is None else n_seg, C.c_void_p(f32), C.c_void_p(u8), seed,
                               step, sample0, None)


def test_entry_point_refuses_bad_tables_before_any_launch():
    good = lambda **kw: N.Segment(**{**dict(offset=0, kind="normal", draw_id=0, B_local=3, inner=7), **kw})  # noqa: E731
    T = lambda segs, nf=64, nu=64: N.SegmentTable(segs, nf, nu)  # noqa: E731
    assert _fill(T([good()]), n_seg=0) < 0 and _fill(T([good()]), n_seg=65) < 0
    assert _fill(T([good(offset=64 - 20)])) < 0                        # 21 floats from 44: past a 64-float buffer
    assert _fill(T([good(kind="keep", keep_p=0.9, offset=50)])) < 0    # ... past the u8 buffer
    assert _fill(T([good(kind=3)])) < 0 and _fill(T([good(kind=-1)])) < 0
    assert _fill(T([good(kind="keep", keep_p=1.5)])) < 0
    assert _fill(T([good(offset=-4)])) < 0 and _fill(T([good(B_local=0)])) < 0 and _fill(T([good(inner=0)])) < 0
    assert _fill(T([good()]), sample0=-1) < 0 and _fill(T([good()]), f32=4100) < 0 and _fill(T([good()]), f32=0) < 0
    for field, v in (("n_outer", 65536), ("draw_id", 65536), ("n_outer", 0), ("draw_id", -1)):
        t = T([good()], nf=1 << 30)
        setattr(t.c_table.seg[0], field, v)  # (the builder itself refuses these: written behind its back)
        assert _fill(t) < 0, field
    t = T([good(), good(offset=24)])
    t.c_table.seg[1].group0 += 1
    assert _fill(t) < 0
    t = T([good()])
    t.c_table.n_groups += 1
    assert _fill(t) < 0
