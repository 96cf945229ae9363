"""The batched ring GEMM (rnn_ops.hip rnn_gemm_kernel) with a NULL operand and without the fp32 store.

x[p] == NULL stands for a zero operand - the first step of a stacked RNN, h_{-1} = 0: the problem's main K tiles are neither
fetched nor multiplied.  The accumulators start at +0 and +0 + (+-0) * w = +0 for finite w, so the result must have the very
bits of the same launch with a buffer of zeros; with no K extension either (nk == 0: the K loop does not run) it must be
act(bias + addend) in the kernel's order of additions.  y[p] == NULL leaves out the fp32 store of that problem only.

Shapes: K = 256 (two K tiles), one per tile route of rnn_fwd_batch / launch_small - 64 x 32 on the 4-stage ring (at most 192
workgroups), 64 x 32 on the 2-stage ring (more; 200 rows: a ragged last tile), 128 x 64 with 8 waves (three problems).
Outputs are prefilled with NaN / 0xFF bytes: an unwritten element shows."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 256
EINVAL = -22
# (tile route, problems, M, N)
SHAPES = [("64x32/4", 1, 64, 64), ("64x32/2", 2, 200, 2048), ("128x64/2", 3, 128, 128)]


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _problems(nprob, M, N, dev):
    """Operands of nprob problems; problem 0 is the one that gets the NULL operand."""
    mk = lambda *s, seed, dt=torch.float32: _rnd(*s, seed=seed).to(dt).to(dev)  # noqa: E731
    d = dict(x=[mk(M, K, seed=10 + p, dt=torch.bfloat16) for p in range(nprob)],
             w=[(_rnd(N, K, seed=30 + p) / math.sqrt(K)).to(torch.bfloat16).to(dev) for p in range(nprob)],
             b=[mk(N, seed=40 + p) for p in range(nprob)], ad=[mk(M, N, seed=50 + p) for p in range(nprob)],
             act=[1] + [0, 1][: nprob - 1])
    d["x"][0] = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 128 - t.shape[1], dtype=t.dtype)], 1).contiguous().to(dev)  # noqa: E731
    d["xe"], d["we"] = pad(_rnd(M, 48, seed=70).to(torch.bfloat16)), pad((_rnd(N, 48, seed=71) / math.sqrt(48)).to(torch.bfloat16))
    d["b2"] = mk(N, seed=73)
    return d


def _launch(d, nprob, M, N, mix, null_x, null_y=False, rc_only=False):
    """One launch; problem 0 with the K extension and no addend (mix "ext") or with an addend and no extension ("addend":
    nk == 0 when its x is NULL); the other problems ordinary (x, bias, addend).  -> (y, yb) lists, NaN-prefilled."""
    from tacorl_amd import _lib, ops

    dev = d["w"][0].device
    nan = lambda dt: torch.full((M, N), float("nan"), device=dev, dtype=dt)  # noqa: E731
    y, yb = [nan(torch.float32) for _ in range(nprob)], [nan(torch.bfloat16) for _ in range(nprob)]
    xs = [None if null_x and p == 0 else d["x"][p] for p in range(nprob)]
    ys = [None if null_y and p == 0 else y[p] for p in range(nprob)]
    pa, none = ops.ptr_array, [None] * (nprob - 1)
    if mix == "ext":
        ad = [None] + d["ad"][1:]
        rc = _lib.lib().tacorl_rnn_linear_fwd_batch_ext(
            nprob, pa(xs), None, pa(d["w"]), pa(d["b"]), pa(ad), None, N, pa(ys), None, pa(yb), None, M, 0, K, N,
            ops.int_array(d["act"]), pa([d["xe"]] + none), None, pa([d["we"]] + none), pa([d["b2"]] + none), ops.stream())
    else:
        rc = _lib.lib().tacorl_rnn_linear_fwd_batch(nprob, pa(xs), pa(d["w"]), pa(d["b"]), pa(d["ad"]), N, pa(ys), pa(yb), M, K, N,
                                                    ops.int_array(d["act"]), ops.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return y, yb


@pytest.mark.parametrize("mix", ["ext", "addend"])
@pytest.mark.parametrize("route,nprob,M,N", SHAPES)
def test_null_operand_equals_zero_buffer(route, nprob, M, N, mix):
    """(at nprob == 3 this is the launch that mixes one NULL and two ordinary problems)"""
    d = _problems(nprob, M, N, _dev())
    y0, yb0 = _launch(d, nprob, M, N, mix, null_x=False)
    y1, yb1 = _launch(d, nprob, M, N, mix, null_x=True)
    for p in range(nprob):
        assert torch.isfinite(y0[p]).all() and torch.isfinite(yb0[p].float()).all(), p
        assert torch.equal(_bits(y1[p]), _bits(y0[p])), (route, mix, p)
        assert torch.equal(_bits(yb1[p]), _bits(yb0[p])), (route, mix, p)
        assert torch.equal(_bits(yb1[p]), _bits(y1[p].to(torch.bfloat16))), p
    if mix == "addend":  # nk == 0: act(bias + addend), the accumulator's +0 first, in the epilogue's order
        z = (torch.zeros(M, N, device=y1[0].device) + d["b"][0]) + d["ad"][0]
        assert torch.equal(_bits(y1[0]), _bits(torch.relu(z)))
    else:  # the extension tile alone: against fp32 torch on the same bf16 operands
        z = torch.relu(d["xe"].float() @ d["we"].float().t() + d["b"][0] + d["b2"])
        assert ((y1[0] - z).norm() / z.norm()).item() < 1e-5


@pytest.mark.parametrize("route,nprob,M,N", SHAPES)
def test_null_y_skips_only_the_fp32_store(route, nprob, M, N):
    d = _problems(nprob, M, N, _dev())
    for null_x in (False, True):
        y0, yb0 = _launch(d, nprob, M, N, "ext", null_x=null_x)
        y1, yb1 = _launch(d, nprob, M, N, "ext", null_x=null_x, null_y=True)
        assert torch.isnan(y1[0]).all(), "problem 0's fp32 buffer must not be written"
        for p in range(nprob):
            assert torch.equal(_bits(yb1[p]), _bits(yb0[p])), (route, p)
            if p:
                assert torch.equal(_bits(y1[p]), _bits(y0[p])), (route, p)


def test_null_operand_with_twin_rows_is_refused():
    from tacorl_amd import _lib, ops

    dev = _dev()
    nprob, M, N = 2, 64, 64
    d = _problems(nprob, M, N, dev)
    x2 = [torch.zeros(M, K, dtype=torch.bfloat16, device=dev) for _ in range(nprob)]
    nan = lambda dt: torch.full((M, N), float("nan"), device=dev, dtype=dt)  # noqa: E731
    y, y2 = [nan(torch.float32) for _ in range(nprob)], [nan(torch.float32) for _ in range(nprob)]
    yb, yb2 = [nan(torch.bfloat16) for _ in range(nprob)], [nan(torch.bfloat16) for _ in range(nprob)]
    pa = ops.ptr_array
    args = lambda xs: (nprob, pa(xs), pa(x2), pa(d["w"]), pa(d["b"]), pa(d["ad"]), pa(d["ad"]), N, pa(y), pa(y2), pa(yb), pa(yb2),  # noqa: E731
                       M, M, K, N, ops.int_array(d["act"]), ops.stream())
    assert _lib.lib().tacorl_rnn_linear_fwd_batch_twin(*args([None, d["x"][1]])) == EINVAL
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in y + y2), "a refused call launches nothing"
    assert _lib.lib().tacorl_rnn_linear_fwd_batch_twin(*args(d["x"])) == 0  # (the zero buffer is what twin launches keep passing)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in y + y2)
