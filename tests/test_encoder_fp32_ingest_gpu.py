"""The fused encoder forward's fp32 CHW source mode (tacorl_encoder_fwd_fused_src) and the TACORL route built on it: the
forward-only images - window frames, next observations - are converted by the encoder's own waves instead of by the pack.
Everything here is BIT identity against the packed route (pack_nchw3_batch + bf16 NHWC source): same rounding, same LDS
image, same kernel behind it.  84 x 84 (the one geometry the mode is built for), tiny image counts."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tacorl_amd import ops  # noqa: E402
from tacorl_amd._lib import call, lib  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 84
IMG = 3 * H * W
NAN_FILL = 0x7FCABCDE  # a NaN no arithmetic produces: an element still holding it was never written


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _prefilled(*shape):
    return torch.full(shape, NAN_FILL, dtype=torch.int32, device=_dev()).view(torch.float32)


def _written_and_equal(a, b):
    return bool((_bits(a) != NAN_FILL).all()) and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def net():
    """One encoder: (fp32 parameter block, packed conv weights)."""
    call("tacorl_hip_init", 0)
    g = torch.Generator(device=_dev()).manual_seed(11)
    off, total = ops.encoder_param_layout()
    p = torch.randn(total, device=_dev(), generator=g) * 0.05
    p[off[6]] = 1.0  # soft-argmax temperature
    pk = torch.empty(lib().tacorl_encoder_fused_wpk_bytes(), dtype=torch.uint8, device=_dev())
    call("tacorl_encoder_pack_weights", 1, ops.ptr_array([p]), ops.ptr_array([pk]), ops.stream())
    return p, pk


def _images(n, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.rand(n, 3, H, W, device=_dev(), generator=g) * 2 - 1


def _pack(src, n, pitch):
    dst = torch.empty(n, H, W, 3, device=_dev(), dtype=torch.bfloat16)
    call("tacorl_pack_images_batch", 1, ops.ptr_array([src]), (C.c_long * 1)(pitch), ops.ptr_array([dst]), ops.int_array([n]), 1, H, W,
         ops.stream())
    return dst


def _table(n=2):
    return torch.zeros(n * lib().tacorl_encoder_src_entry_bytes(), dtype=torch.uint8, device=_dev())


def _fill(tbl, srcs, pitches):
    n, Lg = len(srcs), C.c_long * len(srcs)
    call("tacorl_encoder_src_fill", ops.ptr(tbl), n, ops.ptr_array(srcs), Lg(*pitches), Lg(*[H * W] * n), Lg(*[W] * n), H, W, ops.stream())


def _launch(net, probs, max_wg=0):
    """probs: (packed images or None, table entry address or None, out, act or None, n)"""
    p, pk = net
    k = len(probs)
    call("tacorl_encoder_fwd_fused_src", k, ops.ptr_array([x[0] for x in probs]), ops.ptr_array([x[1] for x in probs]),
         ops.ptr_array([pk] * k), ops.ptr_array([p] * k), ops.ptr_array([x[2] for x in probs]), ops.ptr_array([x[3] for x in probs]),
         ops.int_array([x[4] for x in probs]), H, W, max_wg, ops.stream())


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32).to(_dev())


@pytest.mark.parametrize("n", [1, 2, 7, 17])
def test_fp32_source_is_bit_identical_to_pack_plus_bf16_source(net, n):
    """`out` (prefilled with a marker NaN) of an fp32-source problem equals, bit for bit, the same images through
    pack_nchw3_batch + bf16 source.  The images hold +-0, exact round-to-even ties of bf16 in both directions (a truncating or
    round-half-up conversion fails there, and on half of the U(-1, 1) values anyway), the largest fp32 values that stay
    finite in bf16 and, in the last image when there are two or more, +-FLT_MAX, which round-to-nearest-even turns into
    infinities (that image's features may then be NaN on both routes alike - hence bits, and the marker)."""
    x = _images(n, 100 + n)
    special = _f32([0x00000000, 0x80000000,              # +-0
                    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even downwards / upwards, both signs
                    0x3F807FFF, 0x3F808001,              # just below / above a tie
                    0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF, 0xFF7F7FFF])  # largest values that stay finite in bf16
    flat = x.view(n, -1)
    for i in range(n):
        pos = torch.arange(special.numel(), device=_dev()) * 1777 + 13 * i  # spread over planes, rows and groups
        flat[i, pos % IMG] = special
    if n >= 2:
        flat[n - 1, 5000] = 3.4028234663852886e38
        flat[n - 1, 12001] = -3.4028234663852886e38
    tbl = _table()
    _fill(tbl, [x], [IMG])
    o_pack, o_f32 = _prefilled(n, 32), _prefilled(n, 32)
    _launch(net, [(_pack(x, n, IMG), None, o_pack, None, n)])
    _launch(net, [(None, tbl.data_ptr(), o_f32, None, n)])
    torch.cuda.synchronize()
    assert _written_and_equal(o_f32, o_pack)
    assert torch.isfinite(o_f32[: max(n - 1, 1)]).all()


@pytest.mark.parametrize("budget", [1, 2, 3, 0])
def test_mixed_launch_crosses_format_boundaries(net, budget):
    """Three problems in one launch - bf16 source with saved activations (3 images), fp32 source (5), bf16 source (2) - on
    workgroup budgets 1, 2, 3 and the default: with budget 1 one workgroup crosses both format boundaries.  Outputs and saved
    activations are bit-identical to the all-packed launch on the same budget.  (Through tacorl_encoder_fwd_fused_src, the
    budgeted launch with sources; tacorl_encoder_fwd_fused_wg itself refuses a budget below the problem count.)"""
    xs = [_images(k, 200 + k) for k in (3, 5, 2)]
    xb = [_pack(x, x.shape[0], IMG) for x in xs]
    tbl = _table()
    _fill(tbl, [xs[1]], [IMG])
    res = []
    for entry in (None, tbl.data_ptr()):
        outs = [_prefilled(x.shape[0], 32) for x in xs]
        act = _prefilled(ops.encoder_act_layout(3, H, W)[1])
        _launch(net, [(xb[0], None, outs[0], act, 3), (None if entry else xb[1], entry, outs[1], None, 5), (xb[2], None, outs[2], None, 2)], budget)
        res.append((outs, act))
    torch.cuda.synchronize()
    (oa, aa), (ob, ab) = res
    for a, b in zip(oa, ob):
        assert _written_and_equal(b, a)
    assert torch.equal(_bits(aa), _bits(ab))
    # (saved activations go with the packed source only)
    p, pk = net
    assert lib().tacorl_encoder_fwd_fused_src(1, ops.ptr_array([None]), ops.ptr_array([tbl.data_ptr()]), ops.ptr_array([pk]), ops.ptr_array([p]),
                                              ops.ptr_array([oa[0]]), ops.ptr_array([aa]), ops.int_array([3]), H, W, 0, ops.stream()) != 0


def test_pitched_source_and_table_refill(net):
    """The source is a slice of a larger tensor (image pitch 2 x 3 H W, base not at the tensor's start), and two different
    source tensors go through the SAME table entry in two successive, otherwise identical launches."""
    n = 5
    g = torch.Generator(device=_dev()).manual_seed(31)
    big = [torch.rand(n, 2, 3, H, W, device=_dev(), generator=g) * 2 - 1 for _ in range(2)]
    tbl = _table()
    for t in big:
        src = t[:, 1]
        assert src.stride(0) == 2 * IMG and src.data_ptr() != t.data_ptr()
        _fill(tbl, [src], [src.stride(0)])
        o_f32, o_pack = _prefilled(n, 32), _prefilled(n, 32)
        _launch(net, [(None, tbl.data_ptr(), o_f32, None, n)])
        _launch(net, [(_pack(src, n, src.stride(0)), None, o_pack, None, n)])
        torch.cuda.synchronize()
        assert _written_and_equal(o_f32, o_pack)
    # what the table refuses: a misaligned base, a pitch that is no multiple of four floats, another geometry
    ok = lambda base, pitch, h=H, w=W: lib().tacorl_encoder_src_supported(C.c_void_p(base), pitch, h * w, w, h, w)  # noqa: E731
    base = big[0].data_ptr()
    assert ok(base, IMG) and not ok(base + 4, IMG) and not ok(base, IMG + 2) and not ok(base, 3 * 64 * 64, 64, 64)


# ----------------------------------------------------------------------------------------------- the TACORL step
B, T = 2, 3


def _mod(compute="bf16", graph=False, fold=True):
    import bench

    mod = bench.build_module(_dev(), compute, T, 1)
    mod.fp32_ingest = fold  # (False: the pack route for every image, as before the fp32 source mode)
    if graph:
        mod.enable_graph()
    return mod


def _batch(seed):
    import bench

    return bench.synth_batch(B, T, H, W, _dev(), seed)


def _run(mod, batches, nchw=True):
    """One training step per batch from fixed noise seeds: per step the logged scalars and the latent plan, at the end the
    parameters."""
    per_step = []
    for i, b in enumerate(batches):
        torch.manual_seed(40 + i)
        mod.logged = {}
        mod._step(b, None, optimize=True, log_type="train", nchw=nchw)
        mod._tick_optimizers()
        torch.cuda.synchronize()
        per_step.append(({k: float(v) for k, v in mod.logged.items()}, mod.plan.clone()))
    return per_step, {k: v.detach().clone() for k, v in mod.state_dict().items()}


def _same(a, b):
    (sa, pa), (sb, pb) = a, b
    for (la, plan_a), (lb, plan_b) in zip(sa, sb):
        assert la.keys() == lb.keys() and la
        assert all(la[k] == lb[k] or (la[k] != la[k] and lb[k] != lb[k]) for k in la), {k: (la[k], lb[k]) for k in la if la[k] != lb[k]}
        assert torch.equal(_bits(plan_a), _bits(plan_b))
    assert pa.keys() == pb.keys()
    diff = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not diff, diff[:10]


def test_tacorl_step_equals_the_pack_route():
    """TACORL, B = 2, T = 3, 84 x 84, bf16, three optimiser steps: logged scalars and latent plan of every step and every
    parameter block at the end are bit-identical between the fp32-source route and the forced pack route."""
    batches = [_batch(70 + i) for i in range(3)]
    new, old = _mod(fold=True), _mod(fold=False)
    rn, ro = _run(new, batches), _run(old, batches)
    assert new._folded == ("rgb_static",) and old._folded == ()
    assert all(x.get("src") for x in new.engine.extra_enc) and not any(x.get("src") for x in old.engine.extra_enc)
    _same(rn, ro)
    # the route leaves the window frames and the next observations unpacked; a READER of the buffers still gets them
    assert torch.equal(new.frames["rgb_static"], old.frames["rgb_static"])
    assert torch.equal(new.engine.X3["rgb_static"], old.engine.X3["rgb_static"])


def test_graph_replay_follows_the_batch_tensor():
    """Under graph replay the encoder launch is a captured node: four steps over batch tensors at different addresses (all
    kept alive) equal their eager twins step by step.  A replay that kept the captured source pointer would encode the
    capture's batch again."""
    batches = [_batch(80 + i) for i in range(4)]
    assert len({b["states"]["rgb_static"].data_ptr() for b in batches}) == 4
    graph, eager = _mod(graph=True), _mod()
    rg, re_ = _run(graph, batches), _run(eager, batches)
    assert graph._folded == ("rgb_static",) and len(graph._graphs) == 1
    _same(rg, re_)
    assert not torch.equal(rg[0][-1][1], rg[0][-2][1])  # (the plan does depend on the batch)


def _nhwc(b):
    return {**b, "states": {c: v.permute(0, 1, 3, 4, 2).contiguous() for c, v in b["states"].items()},
            "goal": {c: v.permute(0, 2, 3, 1).contiguous() for c, v in b["goal"].items()}}


def _misaligned(b):
    """The same values in tensors that start four bytes past a 16-byte boundary."""
    def shift(v):
        buf = torch.empty(v.numel() + 4, device=v.device, dtype=v.dtype)
        out = buf[1: 1 + v.numel()].view(v.shape)
        out.copy_(v)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out
    return {**b, "states": {c: shift(v) for c, v in b["states"].items()}, "goal": {c: shift(v) for c, v in b["goal"].items()}}


@pytest.mark.parametrize("case", ["nhwc", "misaligned", "f32"])
def test_ineligible_batches_keep_the_pack_route(case):
    """An NHWC fp32 batch, a batch four bytes off alignment and fp32 compute do not qualify: they take the pack route on their
    own and give what the pack route gives for the same values (the route switch off; for the NHWC and the misaligned batch
    also: the aligned NCHW batch of the same values, packed)."""
    plain = [_batch(90), _batch(91)]
    compute = "f32" if case == "f32" else "bf16"
    given = {"nhwc": [_nhwc(b) for b in plain], "misaligned": [_misaligned(b) for b in plain], "f32": plain}[case]
    nchw = case != "nhwc"
    auto, forced = _mod(compute), _mod(compute, fold=False)
    ra, rf = _run(auto, given, nchw), _run(forced, given, nchw)
    assert auto._folded == () and auto.engine.fp_src == {} and not any(x.get("src") for x in auto.engine.extra_enc)
    _same(ra, rf)
    if case != "f32":
        _same(ra, _run(_mod(compute, fold=False), plain))
