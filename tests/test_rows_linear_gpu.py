"""tacorl_rows_linear2_fwd (csrc/rollout_ops.hip) against the fp64 restatement of tests/rows_linear_ref.py: every element inside
the a-priori fp32 bound on its own operands, padding untouched, rows bit-identical whatever R is and wherever they sit,
flagged rows never read, refusals before any launch."""
import ctypes as C

import pytest
import torch

from tests import rows_linear_ref as RL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22


def _lib():
    from tacorl_amd import _lib

    return _lib


def G():
    return _lib().lib().tacorl_rows_linear2_group()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run(p, act, x2=True, b2=True, flags=True, w1_off=0, ypad=3, rows=None, raw=False):
    """The kernel on problem p (rows: only that row, as an R = 1 call).  Returns (y (R, N) on the CPU, the whole padded y buffer,
    the device copies of x1 / x2) - or the return code alone with raw=True."""
    L = _lib()
    R, K1, K2, N = p["R"], p["K1"], p["K2"], p["N"]
    d = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    x1, xx2 = d(p["x1"]), d(p["x2"]) if x2 else None
    wbuf = torch.zeros(N * K1 + w1_off, device=DEV)
    wbuf[w1_off:] = p["w1"].reshape(-1).to(DEV)
    w1 = wbuf[w1_off:]
    w2, b1 = d(p["w2"]) if x2 else None, d(p["b1"])
    bb2 = d(p["b2"]) if b2 else None
    fl = d(p["flags"]) if (flags and x2) else None
    y = torch.full((R, N + ypad), RL.PAD, device=DEV)
    r0, nr = (0, R) if rows is None else (rows, 1)
    at = lambda t, r: None if t is None else C.c_void_p(t.data_ptr() + r * t.stride(0) * t.element_size())  # noqa: E731
    args = (at(x1, r0), x1.stride(0), K1, _ptr(w1), _ptr(b1), at(xx2, r0), 0 if xx2 is None else xx2.stride(0),
            K2 if xx2 is not None else 0, _ptr(w2), _ptr(bb2), at(fl, r0), at(y, r0), y.stride(0), nr, N, act,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if raw:
        return L.lib().tacorl_rows_linear2_fwd(*args)
    L.call("tacorl_rows_linear2_fwd", *args)
    torch.cuda.synchronize()
    return y[:, :N].cpu(), y.cpu(), (x1.cpu(), None if xx2 is None else xx2.cpu())


def reference(p, act, x2=True, b2=True, flags=True):
    q = dict(p)
    if not x2:
        q["x2"] = q["w2"] = None
    if not b2:
        q["b2"] = None
    if not flags:
        q["flags"] = None
    y, scale = RL.restate(q, act)
    return y, RL.bound(q, scale)


VARIANTS = [dict(), dict(b2=False), dict(x2=False), dict(flags=False), dict(w1_off=1), dict(x2=False, b2=False, w1_off=1)]


@pytest.mark.parametrize("K1,K2", RL.SHAPES_K)
@pytest.mark.parametrize("Rk", ["1", "G-1", "G", "G+1", "64"])
def test_every_element_inside_the_apriori_bound(K1, K2, Rk):
    g = G()
    R = {"1": 1, "G-1": g - 1, "G": g, "G+1": g + 1, "64": 64}[Rk]
    worst = 0.0
    for N in RL.SHAPES_N:
        p = RL.problem(R, K1, K2, N, seed=1000 * K1 + 10 * N + R, flag_rows=[r for r in (0, R - 2) if 0 <= r < R] if K2 else ())
        for act in (RL.ACT_NONE, RL.ACT_RELU):
            for v in VARIANTS:
                if K2 == 0 and (v.get("x2", True) is False or v.get("flags", True) is False):
                    continue  # (nothing to leave out)
                kw = {k: v[k] for k in ("x2", "b2", "flags") if k in v}
                y, ybuf, (x1, x2) = run(p, act, **v)
                ref, bnd = reference(p, act, **kw)
                err = (y.double() - ref).abs()
                worst = max(worst, (err / bnd).max().item())
                assert bool((err <= bnd).all()), (N, act, v, (err / bnd).max().item())
                assert bool((ybuf[:, N:] == RL.PAD).all()), "the padding columns of y were written"
                assert torch.equal(x1, p["x1"]) and (x2 is None or torch.equal(x2, p["x2"]))
    print(f"R {R} K ({K1}, {K2}): worst |err| / bound = {worst:.3g}")


def test_real_shape_inside_the_bound():
    p = RL.problem(2, 2048, 2048, 2048, seed=5, flag_rows=(1,))
    for act in (RL.ACT_NONE, RL.ACT_RELU):
        y, ybuf, _ = run(p, act)
        ref, bnd = reference(p, act)
        err = (y.double() - ref).abs()
        print(f"act {act}: worst |err| / bound = {(err / bnd).max().item():.3g}")
        assert bool((err <= bnd).all()) and bool((ybuf[:, 2048:] == RL.PAD).all())


@pytest.mark.parametrize("K1,K2,N", [(45, 72, 182), (257, 259, 7), (48, 0, 240)])
def test_rows_are_bit_identical_alone_and_in_a_batch(K1, K2, N):
    R = G() + 1
    p = RL.problem(R, K1, K2, N, seed=77, flag_rows=(1, R - 1) if K2 else ())
    for w1_off in (0, 1):
        y, _, _ = run(p, RL.ACT_RELU, w1_off=w1_off)
        for r in range(R):
            alone, _, _ = run(p, RL.ACT_RELU, w1_off=w1_off, rows=r)
            assert torch.equal(alone[r], y[r]), (r, w1_off)


def test_flagged_rows_are_not_read():
    R = G() + 1
    p = RL.problem(R, 48, 72, 182, seed=9, flag_rows=(2, R - 1))
    zeroed = dict(p, x2=p["x2"].clone(), flags=None)
    zeroed["x2"][[2, R - 1]] = 0.0  # (whole rows, padding included: the kernel reads the first K2 columns)
    want, _, _ = run(zeroed, RL.ACT_NONE)
    poisoned = dict(p, x2=p["x2"].clone())
    poisoned["x2"][[2, R - 1]] = float("nan")
    got, _, _ = run(poisoned, RL.ACT_NONE)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)  # the flagged rows as with zeros, the unflagged neighbours unchanged
    plain, _, _ = run(dict(p, flags=None), RL.ACT_NONE)
    keep = [r for r in range(R) if r not in (2, R - 1)]
    assert torch.equal(got[keep], plain[keep]) and not torch.equal(got[2], plain[2])


def test_refusals_leave_the_output_untouched():
    L = _lib().lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x1, x2 = torch.randn(64, 48, device=DEV), torch.randn(64, 72, device=DEV)
    w1, w2, b = torch.randn(72, 48, device=DEV), torch.randn(72, 72, device=DEV), torch.randn(72, device=DEV)
    y = torch.full((64, 72), RL.PAD, device=DEV)
    x2_before = x2.clone()
    f = lambda R, yy=y, ww1=w1: L.tacorl_rows_linear2_fwd(  # noqa: E731
        _ptr(x1), 48, 48, _ptr(ww1), _ptr(b), _ptr(x2), 72, 72, _ptr(w2), _ptr(b), None, _ptr(yy), 72, R, 72, RL.ACT_RELU, st)
    assert f(0) == EINVAL and f(65) == EINVAL
    assert f(64, yy=x2) == EINVAL            # y aliasing x2
    assert f(64, ww1=None) == EINVAL         # null w1
    assert L.tacorl_rows_linear2_supported(0, 48, 72, 72) == 0 and L.tacorl_rows_linear2_supported(65, 48, 72, 72) == 0
    assert L.tacorl_rows_linear2_supported(64, 45, 0, 1) == 1 and L.tacorl_rows_linear2_supported(1, 0, 0, 1) == 0
    torch.cuda.synchronize()
    assert bool((y == RL.PAD).all()) and torch.equal(x2, x2_before)
    assert f(64) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and not bool((y == RL.PAD).any())
