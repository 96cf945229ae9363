"""tacorl_rows_mlp_fwd (csrc/rollout_ops.hip) against the fp64 restatement of tests/rows_policy_ref.py: every hidden layer - read
from the workspace - inside the a-priori bound on the kernel's own input of that layer, every action element inside its bound,
the gripper column exact in every row, padding untouched, rows bit-identical whatever R is and wherever they sit, both
neurons-per-wave arms bit-identical, refusals before any launch."""
import ctypes as C

import pytest
import torch

from tests import rows_policy_ref as RP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
PLAIN, POLICY = 0, 1


def _L():
    from tacorl_amd import _lib

    return _lib


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * off)


class Chain:
    """Problem p on the device: x (64, E + 3) with the pad columns at PAD, one tensor per weight and bias."""

    def __init__(self, p):
        self.p = p
        self.x = p["x"].to(DEV).contiguous()
        self.W = [w.to(DEV).contiguous() for w in p["W"]]
        self.b = [v.to(DEV).contiguous() for v in p["b"]]
        n = len(self.W)
        self.dims, self.w_arr, self.b_arr = (C.c_int * (n + 1))(*p["dims"]), (C.c_void_p * n)(*[w.data_ptr() for w in self.W]), \
            (C.c_void_p * n)(*[v.data_ptr() for v in self.b])

    def args(self, R, mode, y_t, ws_t, acts_l=None, row0=0, npw=0, **over):
        p = self.p
        n = len(self.W)
        a = dict(x=_ptr(self.x, row0 * self.x.stride(0)), ldx=self.x.stride(0), n=n, dims=self.dims, w=self.w_arr, b=self.b_arr,
                 acts=(C.c_int * n)(*(acts_l or p["acts"])), ws=_ptr(ws_t), y=_ptr(y_t), ldy=y_t.stride(0), R=R, mode=mode, Ac=p["Ac"],
                 dg=int(p["dg"]), npw=npw)
        a.update(over)
        return (a["x"], a["ldx"], a["n"], a["dims"], a["w"], a["b"], a["acts"], a["ws"], a["y"], a["ldy"], a["R"], a["mode"],
                a["Ac"], a["dg"], a["npw"], C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self, R, mode=POLICY, acts=None, row0=0, npw=0):
        """-> (y (R, width) on the CPU, the whole padded y buffer, the hidden layers [l] (R, H) from the workspace)."""
        p = self.p
        width = p["A"] if mode == POLICY else p["dims"][-1]
        y = torch.full((R, width + 3), RP.PAD, device=DEV)
        ws = torch.full((max(p["L"] * R * p["H"], 1),), RP.PAD, device=DEV)
        _L().call("tacorl_rows_mlp_fwd", *self.args(R, mode, y, ws, acts, row0, npw))
        torch.cuda.synchronize()
        hid = [ws[l * R * p["H"]: (l + 1) * R * p["H"]].view(R, p["H"]).cpu() for l in range(p["L"])]
        return y[:, :width].cpu(), y.cpu(), hid


_chains = {}


def chain(shape, head):
    if (shape, head) not in _chains:
        _chains[(shape, head)] = Chain(RP.problem(shape, head))
    return _chains[(shape, head)]


def check(c, R, y, ybuf, hid, mode=POLICY, last_act=None):
    """Every layer on the kernel's own input of that layer; returns the worst |err| / bound."""
    p = c.p
    worst = 0.0
    h = p["x"][:R, :p["E"]]
    for l in range(p["L"]):
        ref, bnd = RP.layer_ref(p, l, h)
        err = (hid[l].double() - ref).abs()
        worst = max(worst, (err / bnd).max().item())
        assert bool((err <= bnd).all()), (R, l, (err / bnd).max().item())
        h = hid[l]
    if mode == POLICY:
        ref, bnd, _, _ = RP.action_ref(p, h)
        Ac = p["Ac"]
        err = (y[:, :Ac].double() - ref[:, :Ac]).abs()
        assert bool((err <= bnd).all()), (R, "action", (err / bnd).max().item())
        assert torch.equal(y[:, Ac:].double(), ref[:, Ac:]), (R, "gripper", y[:, Ac:].T, ref[:, Ac:].T)
    else:
        ref, bnd = RP.layer_ref(p, p["L"], h, last_act)
        err = (y.double() - ref).abs()
        assert bool((err <= bnd).all()), (R, "plain", (err / bnd).max().item())
    worst = max(worst, (err / bnd).max().item())
    assert bool((ybuf[:, y.shape[1]:] == RP.PAD).all()), "the padding columns of y were written"
    return worst


@pytest.mark.parametrize("head", RP.HEADS)
@pytest.mark.parametrize("shape", RP.SHAPES)
def test_policy_action_inside_the_bounds(shape, head):
    c = chain(shape, head)
    worst = 0.0
    for R in RP.ROWS:
        worst = max(worst, check(c, R, *c.run(R)))
        assert torch.equal(c.x.cpu(), c.p["x"])
    print(f"{shape} {head}: worst |err| / bound = {worst:.3g}")


def test_configured_shape_inside_the_bounds():
    c = chain(RP.REAL_SHAPE, RP.HEADS[0])
    print(f"{RP.REAL_SHAPE}: worst |err| / bound = {check(c, RP.REAL_ROWS, *c.run(RP.REAL_ROWS)):.3g}")


@pytest.mark.parametrize("last_act", [RP.ACT_TANH, RP.ACT_NONE])
@pytest.mark.parametrize("shape", RP.SHAPES)
def test_plain_mode_inside_the_bounds(shape, last_act):
    """The last layer as an ordinary one (the goal encoder's Tanh or no activation): all 2 Ac + 2 neurons of the head."""
    c = chain(shape, RP.HEADS[0])
    acts = c.p["acts"][:-1] + [last_act]
    for R in (1, 3, 9, 64):
        y, ybuf, hid = c.run(R, mode=PLAIN, acts=acts)
        assert y.shape == (R, c.p["dims"][-1])
        check(c, R, y, ybuf, hid, mode=PLAIN, last_act=last_act)


@pytest.mark.parametrize("shape,head", [(RP.SHAPES[0], RP.HEADS[0]), (RP.SHAPES[1], RP.HEADS[1])])
def test_rows_are_bit_identical_whatever_r_and_place(shape, head):
    c = chain(shape, head)
    full, _, hid = c.run(17)
    for R in (1, 2, 3, 5, 8, 9, 16, 64):
        y, _, h = c.run(R)
        n = min(R, 17)
        assert torch.equal(y[:n], full[:n]), R
        assert all(torch.equal(h[l][:n], hid[l][:n]) for l in range(c.p["L"])), R
    for r in range(17):  # the row alone, as an R = 1 call; and as row 0 of a batch that starts there
        alone, _, _ = c.run(1, row0=r)
        assert torch.equal(alone[0], full[r]), r
    shifted, _, _ = c.run(9, row0=5)
    assert torch.equal(shifted, full[5:14])
    for npw in (1, 2):  # a neuron's summation order does not depend on how many neurons its wave serves
        y, _, h = c.run(17, npw=npw)
        assert torch.equal(y, full) and all(torch.equal(a, b) for a, b in zip(h, hid)), npw


def test_refusals_leave_the_output_untouched():
    L = _L().lib()
    c = chain(RP.SHAPES[0], RP.HEADS[0])
    p = c.p
    y = torch.full((64, p["A"] + 3), RP.PAD, device=DEV)
    ws = torch.full((p["L"] * 64 * p["H"],), RP.PAD, device=DEV)
    f = lambda R=8, mode=POLICY, yy=y, wss=ws, **over: L.tacorl_rows_mlp_fwd(*c.args(R, mode, yy, wss, **over))  # noqa: E731
    n = len(c.W)
    assert f(R=0) == EINVAL and f(R=65) == EINVAL                                    # R outside 1..64
    assert f(n=0) == EINVAL and f(n=9) == EINVAL                                     # layer count outside 1..8
    assert f(x=None) == EINVAL and f(y=None) == EINVAL and f(ws=None) == EINVAL      # null pointers
    assert f(w=None) == EINVAL and f(b=None) == EINVAL and f(dims=None) == EINVAL and f(acts=None) == EINVAL
    null_w = (C.c_void_p * n)(*([c.W[0].data_ptr()] + [None] * (n - 1)))
    assert f(w=null_w) == EINVAL
    assert f(x=C.c_void_p(c.x.data_ptr() + 2)) == EINVAL                             # not 4-byte aligned
    assert f(y=C.c_void_p(y.data_ptr() + 1)) == EINVAL
    odd_b = (C.c_void_p * n)(*([c.b[0].data_ptr() + 2] + [v.data_ptr() for v in c.b[1:]]))
    assert f(b=odd_b) == EINVAL
    assert f(ldx=p["E"] - 1) == EINVAL and f(ldy=p["A"] - 1) == EINVAL               # a leading dimension below its width
    assert f(mode=PLAIN, ldy=p["dims"][-1] - 1) == EINVAL
    assert f(Ac=0) == EINVAL and f(Ac=-3) == EINVAL                                  # Ac < 1
    assert f(Ac=p["Ac"] + 1) == EINVAL                                               # head narrower than 2 Ac + 2
    narrow = (C.c_int * (n + 1))(*(p["dims"][:-1] + [2 * p["Ac"] + 1]))
    assert f(dims=narrow) == EINVAL
    assert f(mode=2) == EINVAL and f(npw=3) == EINVAL and f(acts=(C.c_int * n)(*([RP.ACT_SILU] * (n - 1) + [7]))) == EINVAL
    assert f(y=_ptr(c.x), ldy=c.x.stride(0)) == EINVAL                               # output overlapping the input
    assert f(ws=_ptr(c.x)) == EINVAL and f(ws=_ptr(y)) == EINVAL                     # workspace overlapping input / output
    assert f(y=_ptr(c.W[1]), ldy=p["A"]) == EINVAL                                   # output overlapping a weight
    sup = lambda R, nl=n, Ac=p["Ac"], dg=1, mode=POLICY: L.tacorl_rows_mlp_supported(R, nl, c.dims, mode, Ac, dg)  # noqa: E731
    assert sup(1) == 1 and sup(64) == 1 and sup(0) == 0 and sup(65) == 0 and sup(8, nl=0) == 0 and sup(8, Ac=0) == 0
    assert sup(8, Ac=p["Ac"] + 1) == 0 and sup(8, Ac=p["Ac"] + 1, dg=0) == 1 and sup(8, mode=PLAIN, Ac=0, dg=0) == 1
    torch.cuda.synchronize()
    assert bool((y == RP.PAD).all()) and bool((ws == RP.PAD).all()) and torch.equal(c.x.cpu(), p["x"])
    assert f() == 0
    torch.cuda.synchronize()
    assert bool((y[:8, :p["A"]] != RP.PAD).all()) and bool((y[8:] == RP.PAD).all()) and bool((y[:, p["A"]:] == RP.PAD).all())
