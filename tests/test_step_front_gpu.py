"""TACORL's step front as a graph node fed by a device table (tacorl_step_front, encoder_stage.FrontTable): the kernel against
today's entry points bit for bit, the table following the batch under graph replay, the skipped fill, and the batches that
keep today's launches.  84 x 84 (the fp32-source route's geometry), B = 2 or 3, windows of 2 or 3 frames."""
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
SENTINEL = 0x7FCA  # a bf16 NaN pattern no image value rounds to: an element still holding it was never written
DT = {"float32": (torch.float32, 0), "int64": (torch.int64, 1), "int32": (torch.int32, 2), "bool": (torch.bool, 3)}


def _dev():
    return torch.device("cuda:0")


def _u(*shape, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.rand(*shape, device=_dev(), generator=g) * 2 - 1


def _disp(B, kind, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    d = torch.randint(0, 3, (B,), device=_dev(), generator=g)  # 0, 1, 2: about a third are "1"
    return (d == 1) if kind == "bool" else d.to(DT[kind][0])


def _table():
    return torch.zeros(lib().tacorl_step_front_table_bytes(), dtype=torch.uint8, device=_dev())


def _front(tbl, srcs, jobs, disp, dd, reward, done, B, acts, acts_dst):
    """assemble + fill + launch through the C ABI; jobs: (src address, pitch, dst address, n)."""
    P, Lg = C.c_void_p, C.c_long
    ns, nj = len(srcs), len(jobs)
    host = C.create_string_buffer(tbl.numel())
    n_acts = acts.numel() if acts is not None else 0
    call("tacorl_step_front_assemble", host, ns, (P * ns)(*[s for s, _ in srcs]), (Lg * ns)(*[p for _, p in srcs]), nj,
         (P * nj)(*[j[0] for j in jobs]), (Lg * nj)(*[j[1] for j in jobs]), (P * nj)(*[j[2] for j in jobs]),
         (C.c_int * nj)(*[j[3] for j in jobs]), ops.ptr(disp), dd, ops.ptr(reward), ops.ptr(done), B, ops.ptr(acts), ops.ptr(acts_dst),
         n_acts, H, W)
    call("tacorl_step_front_fill", ops.ptr(tbl), host, ops.stream())
    call("tacorl_step_front", ops.ptr(tbl), nj, max([j[3] for j in jobs], default=0), B, n_acts, H, W, ops.stream())


@pytest.fixture(scope="module")
def window():
    """B = 3, T = 2: the window, the goal, and [obs; goal] packed by tacorl_pack_images_batch into slots 0 and 1 of a
    three-slot buffer whose every other element keeps the sentinel."""
    call("tacorl_hip_init", 0)
    B, T = 3, 2
    states, goal = _u(B, T, 3, H, W, seed=1), _u(B, 3, H, W, seed=2)
    # exact bf16 round-to-even ties, +-0 and the largest finite values, as the pack's own tests use
    special = torch.tensor([0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x7F7F0000,
                            0xFF7F0000], dtype=torch.int64).to(torch.int32).view(torch.float32).to(_dev())
    states.view(-1)[torch.arange(special.numel(), device=_dev()) * 1777 + 5] = special
    goal.view(-1)[torch.arange(special.numel(), device=_dev()) * 911 + 3] = special
    want = torch.full((3 * B, H, W, 3), SENTINEL, dtype=torch.int16, device=_dev()).view(torch.bfloat16)
    slot = B * IMG * 2
    call("tacorl_pack_images_batch", 2, ops.ptr_array([states, goal]), (C.c_long * 2)(T * IMG, IMG),
         ops.ptr_array([want.data_ptr(), want.data_ptr() + slot]), ops.int_array([B, B]), 1, H, W, ops.stream())
    torch.cuda.synchronize()
    return B, T, states, goal, want


@pytest.mark.parametrize("with_acts", [True, False])
@pytest.mark.parametrize("kind", list(DT))
def test_kernel_equals_pack_plus_stage_transition(window, kind, with_acts):
    """One tacorl_step_front launch against tacorl_pack_images_batch + tacorl_stage_transition: obs is the strided view of the
    window (pitch T * 3HW), goal is contiguous; X3's two packed slots, reward, done and the action window bit-identical, the
    third slot's sentinel untouched."""
    B, T, states, goal, want = window
    disp, dd = _disp(B, kind, 7), DT[kind][1]
    acts = _u(B, T, 7, seed=9) if with_acts else None
    n_acts = acts.numel() if with_acts else 0
    ref = [torch.full((B,), -7.0, device=_dev()), torch.full((B,), -7.0, device=_dev()), torch.full((B, T, 7), -7.0, device=_dev())]
    got = [t.clone() for t in ref]
    call("tacorl_stage_transition", ops.ptr(disp), dd, ops.ptr(ref[0]), ops.ptr(ref[1]), B, ops.ptr(acts),
         ops.ptr(ref[2]) if with_acts else None, n_acts, ops.stream())
    x3 = torch.full((3 * B, H, W, 3), SENTINEL, dtype=torch.int16, device=_dev()).view(torch.bfloat16)
    slot = B * IMG * 2
    srcs = [(states.data_ptr(), IMG), (states.data_ptr() + 4 * (T - 1) * IMG, T * IMG)]
    jobs = [(states.data_ptr(), T * IMG, x3.data_ptr(), B), (goal.data_ptr(), IMG, x3.data_ptr() + slot, B)]
    _front(_table(), srcs, jobs, disp, dd, got[0], got[1], B, acts, got[2] if with_acts else None)
    torch.cuda.synchronize()
    assert torch.equal(x3.view(torch.int16), want.view(torch.int16))
    assert bool((x3.view(torch.int16)[2 * B:] == SENTINEL).all()) and not bool((x3.view(torch.int16)[: 2 * B] == SENTINEL).any())
    for g, r in zip(got, ref):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32))
    assert torch.equal(got[0], (disp == 1).float()) and bool((got[2] == (acts if with_acts else -7.0)).all())


@pytest.mark.parametrize("kind", list(DT))
def test_transition_rows_cross_a_block(kind):
    """B = 257: the row index crosses a 256-thread block (no pack job, an action window of 257 * 2 * 7 elements)."""
    call("tacorl_hip_init", 0)
    B, T = 257, 2
    disp, dd, acts = _disp(B, kind, 17), DT[kind][1], _u(B, T, 7, seed=19)
    ref = [torch.full((B + 3,), -7.0, device=_dev()), torch.full((B + 3,), -7.0, device=_dev()), torch.full((B * T * 7 + 5,), -7.0, device=_dev())]
    got = [t.clone() for t in ref]
    call("tacorl_stage_transition", ops.ptr(disp), dd, ops.ptr(ref[0]), ops.ptr(ref[1]), B, ops.ptr(acts), ops.ptr(ref[2]), acts.numel(),
         ops.stream())
    _front(_table(), [], [], disp, dd, got[0], got[1], B, acts, got[2])
    torch.cuda.synchronize()
    for g, r in zip(got, ref):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32))
    assert torch.equal(got[0][:B], (disp == 1).float()) and bool((got[0][B:] == -7.0).all()) and bool((got[2][B * T * 7:] == -7.0).all())


# ----------------------------------------------------------------------------------------------- the TACORL step
B, T = 2, 3


def _mod(compute="bf16", graph=False, fold=True):
    import bench

    mod = bench.build_module(_dev(), compute, T, 1)
    mod.fp32_ingest = fold
    if graph:
        mod.enable_graph()
    return mod


def _batch(seed, b=B, hw=H):
    import bench

    return bench.synth_batch(b, T, hw, hw, _dev(), seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step(mod, b, seed, nchw=True):
    torch.manual_seed(seed)
    mod.logged = {}
    mod._step(b, None, optimize=True, log_type="train", nchw=nchw)
    mod._tick_optimizers()
    torch.cuda.synchronize()
    return {k: float(v) for k, v in mod.logged.items()}, mod.plan.clone()


def _run(mod, batches, nchw=True):
    return [_step(mod, b, 40 + i, nchw) for i, b in enumerate(batches)], {k: v.detach().clone() for k, v in mod.state_dict().items()}


def _same(a, b):
    (sa, pa), (sb, pb) = a, b
    for (la, plan_a), (lb, plan_b) in zip(sa, sb):
        assert la.keys() == lb.keys() and la
        assert all(la[k] == lb[k] or (la[k] != la[k] and lb[k] != lb[k]) for k in la), {k: (la[k], lb[k]) for k in la if la[k] != lb[k]}
        assert torch.equal(_bits(plan_a), _bits(plan_b))
    assert pa.keys() == pb.keys()
    diff = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not diff, diff[:10]


def test_table_follows_the_batch_under_graph_replay():
    """Four steps over batches at four distinct addresses (all alive), then four more over the SAME tensor objects with their
    contents rewritten in place: the graph module (one capture, the front a captured node) equals its eager twin and the
    forced pack route in every logged scalar, the plan and all parameters, bit for bit."""
    batches = [_batch(80 + i) for i in range(4)]
    assert len({b["states"]["rgb_static"].data_ptr() for b in batches}) == 4
    graph, eager, packed = _mod(graph=True), _mod(), _mod(fold=False)
    rg, re_, rp = _run(graph, batches), _run(eager, batches), _run(packed, batches)
    assert graph._front and eager._front and not packed._front and len(graph._graphs) == 1
    _same(rg, re_)
    _same(rg, rp)
    assert not torch.equal(rg[0][-1][1], rg[0][-2][1])  # (the plan does depend on the batch)
    # the same objects, other contents: the node reads the contents every step
    fresh = [_batch(90 + i) for i in range(4)]
    for old, new in zip(batches, reversed(fresh)):
        for k in ("states", "goal"):
            old[k]["rgb_static"].copy_(new[k]["rgb_static"])
        old["actions"].copy_(new["actions"])
        old["disp"].copy_(new["disp"])
    rg2, re2, rp2 = _run(graph, batches), _run(eager, batches), _run(packed, batches)
    assert len(graph._graphs) == 1
    _same(rg2, re2)
    _same(rg2, rp2)
    assert any(a[0] != b[0] for a, b in zip(rg[0], rg2[0]))  # (the outputs followed the contents)
    # reward / done / the action window and the packed [obs; goal] are what the old entry points leave
    assert torch.equal(graph.reward, packed.reward) and torch.equal(graph.engine.done, packed.engine.done)
    assert torch.equal(graph.acts, packed.acts)
    assert torch.equal(graph.engine.X3["rgb_static"], packed.engine.X3["rgb_static"])


WATCHED = ("tacorl_pack_images", "tacorl_stage_transition", "tacorl_step_front", "tacorl_encoder_src_fill")


class Recorder:
    """`call` replaced on every loaded tacorl_amd module that has the name by a recorder that forwards to the real entry
    point; a record is (entry point, issued on the default stream?)."""

    def __init__(self, monkeypatch):
        import tacorl_amd.modules.tacorl.tacorl  # noqa: F401
        from tacorl_amd import _lib

        self.real, self.raw = _lib.call, []
        for name, mod in list(sys.modules.items()):
            if name.startswith("tacorl_amd") and mod is not None and hasattr(mod, "call"):
                monkeypatch.setattr(mod, "call", self.call)

    def call(self, name, *a):
        if name.startswith(WATCHED) and not name.endswith(("_assemble", "_offsets")):
            self.raw.append((name[len("tacorl_"):], torch.cuda.current_stream(_dev()) == torch.cuda.default_stream(_dev())))
        return self.real(name, *a)

    def take(self):
        out, self.raw = self.raw, []
        return out


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def test_fill_is_skipped_while_nothing_moved(rec):
    """Eager steps, so every launch passes the recorder: the first step fills the table, a second step on the same tensors
    does not, tensors at a new address fill once, and after a reallocation (another B) the next step fills again.  The eager
    pack, tacorl_stage_transition and the encoder's own source fill are gone on this route, on every step."""
    mod = _mod()
    a, b = _batch(60), _batch(61)
    assert a["states"]["rgb_static"].data_ptr() != b["states"]["rgb_static"].data_ptr()
    front, fill = ("step_front", True), ("step_front_fill", True)
    _step(mod, a, 1)
    assert rec.take() == [fill, front]
    _step(mod, a, 2)
    assert rec.take() == [front]
    a["states"]["rgb_static"].mul_(0.5)  # (contents, not addresses)
    _step(mod, a, 3)
    assert rec.take() == [front]
    _step(mod, b, 4)
    assert rec.take() == [fill, front]
    _step(mod, b, 5)
    assert rec.take() == [front]
    _step(mod, a, 6)
    assert rec.take() == [fill, front]
    big = _batch(62, b=B + 1)  # _ensure_seq / ensure_batch reallocate
    _step(mod, big, 7)
    assert rec.take() == [fill, front]
    _step(mod, big, 8)
    assert rec.take() == [front]
    # another caller on the same module keeps today's launches, and the step's next table is filled again
    mod._stage_frames(big, None)  # (as get_pr_latent_plan stages them)
    torch.cuda.synchronize()
    assert rec.take() == [("stage_transition", False), ("pack_images_window_batch", True)]
    _step(mod, big, 9)
    assert rec.take() == [fill, front]
    # the step split into graph segments (several ranks, eager collectives between them) keeps today's eager front
    mod._force_graph_split = True
    _step(mod, big, 10)
    assert rec.take() == [("stage_transition", False), ("encoder_src_fill", True), ("pack_images_batch", True)]
    assert mod._front is False and mod._folded == ("rgb_static",)


def _nhwc(b):
    return {**b, "states": {c: v.permute(0, 1, 3, 4, 2).contiguous() for c, v in b["states"].items()},
            "goal": {c: v.permute(0, 2, 3, 1).contiguous() for c, v in b["goal"].items()}}


def _misaligned(b):
    def shift(v):
        buf = torch.empty(v.numel() + 4, device=v.device, dtype=v.dtype)
        out = buf[1: 1 + v.numel()].view(v.shape)
        out.copy_(v)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out
    return {**b, "states": {c: shift(v) for c, v in b["states"].items()}, "goal": {c: shift(v) for c, v in b["goal"].items()}}


def _uint8(b):
    q = lambda v: ((v + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)  # noqa: E731
    return {**b, "states": {c: q(v).permute(0, 1, 3, 4, 2).contiguous() for c, v in b["states"].items()},
            "goal": {c: q(v).permute(0, 2, 3, 1).contiguous() for c, v in b["goal"].items()}}


SMALL, ONE_BY_ONE = ("stage_transition", False), [("pack_images", True)] * 4
# literals: the launches of the eager front as they stood before the front table existed (transition + noise on the side
# stream, the packs on the step's stream) - tests/test_image_ingest_gpu.py pins the same plans with their arguments at 36 x 36
TODAY = {
    "nhwc": [SMALL] + ONE_BY_ONE,                               # no vector pack for NHWC: window, obs, goal, next one by one
    "misaligned": [SMALL] + ONE_BY_ONE,                         # four bytes off a 16-byte boundary: the same
    "f32": [SMALL, ("pack_images_window_batch", True)],         # fp32 compute: not the fused kernel's route
    "uint8": [SMALL, ("pack_images_u8_batch", True)],           # the dataset's frames
    "36x36": [SMALL, ("pack_images_window_batch", True)],       # a geometry the fp32 source mode is not built for
}


@pytest.mark.parametrize("case", list(TODAY))
def test_ineligible_batches_keep_todays_launches(rec, case):
    mod = _mod("f32" if case == "f32" else "bf16")
    plain = _batch(70, hw=36 if case == "36x36" else H)
    given = {"nhwc": _nhwc, "misaligned": _misaligned, "uint8": _uint8}.get(case, lambda b: b)(plain)
    for seed in (1, 2):
        _step(mod, given, seed, nchw=case != "nhwc")
        assert rec.take() == TODAY[case]
    assert mod._front is False and mod.front_tbl.shadow is None
