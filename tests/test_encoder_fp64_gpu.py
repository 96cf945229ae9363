"""The image encoder's kernels (encoder_fused.hip, encoder_ring.hip, encoder_bwd_fused.hip and the per-layer path of
dense_ops.hip) per image, per layer and per gradient slice against the fp64 restatement of tests/encoder_ref.py, on inputs
that make the encoder non-degenerate (structured images, a peaked soft-argmax: tests/test_encoder_ref_cpu.py).

  C1 / C2  every saved activation, element by element, against the fp64 stage evaluated on the kernel's own saved input:
           |got - ref| <= 2 K 2^-24 (sum |x||w| + |b|), the a-priori bound of an fp32 sum in any order (+ 1 bf16 ulp where
           the value is stored as bf16); the soft-argmax at 4 x plain fp32 torch's error on the same y3
  C3       every image's output against the end-to-end reference, at 4 x the fp32 rounded oracle's worst image
  C4       the same image at several places of a launch: bit-identical rows and saved activations, also under workgroup budgets
  C5       logits past exp's fp32 range
  D1       every gradient per output channel (conv weights: also per kernel tap) against fp64, three paths, accumulate both ways
  D2       the gradients of a problem equal the sum of its two halves' up to the fp32 sum's a-priori bound
  D3       the entry points the engine calls (pack -> head -> conv, fc_wgrad; conv_parts) equal the composite bit for bit

Every bound comes from tests/encoder_ref.py; every measured number goes to golden_util.record_margin
(tools/encoder_margins_md.py -> profiles/encoder_margins.md).  A test collects all its figures before it asserts."""
import pytest
import torch

from tests import encoder_ref as R
from tests.golden_util import gradient_floor, record_margin

pytestmark = pytest.mark.gpu

GEOMS = pytest.mark.parametrize("H,W", R.GEOMETRIES)
EINVAL, ENOMEM = -22, -12
STAGES = ["y1", "y2", "y3", "sa", "fc1"]
_floors = {}


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _upload(Ps, dev):
    """fp32 parameter blocks and the fused forward's packed weights, one pair per DISTINCT parameter set."""
    from tacorl_amd import _lib, blocks, ops

    flats, packed = [], []
    for P in Ps:
        flat = torch.zeros(blocks.encoder_size(), device=dev)
        blocks.load_named(blocks.encoder_views(flat), P)
        flats.append(flat)
        packed.append(torch.empty(_lib.lib().tacorl_encoder_fused_wpk_bytes(), dtype=torch.uint8, device=dev))
    ops.call("tacorl_encoder_pack_weights", len(Ps), ops.ptr_array(flats), ops.ptr_array(packed), ops.stream())
    return flats, packed


def _images(imgs, dev, path):
    x = [i.permute(0, 2, 3, 1).contiguous().to(dev) for i in imgs]
    return x if path == "generic_f32" else [i.to(torch.bfloat16) for i in x]


def _forward(path, H, W, flats, packed, imgs_d, budget=None):
    """-> (outputs, saved-activation blocks), both pre-filled with NaN."""
    from tacorl_amd import _lib, ops

    n = [i.shape[0] for i in imgs_d]
    dev = imgs_d[0].device
    outs = [torch.full((k, 32), float("nan"), device=dev) for k in n]
    acts = [torch.full((ops.encoder_act_layout(k, H, W)[1],), float("nan"), device=dev) for k in n]
    if path == "fused":
        assert _lib.lib().tacorl_encoder_fused_supported(H, W) == 1 and _lib.lib().tacorl_encoder_fused_act_format(H, W) == 1
        args = [len(n), ops.ptr_array(imgs_d), ops.ptr_array(packed), ops.ptr_array(flats), ops.ptr_array(outs), ops.ptr_array(acts),
                ops.int_array(n), H, W]
        if budget is None:
            ops.call("tacorl_encoder_fwd_fused", *args, ops.stream())
        else:
            ops.call("tacorl_encoder_fwd_fused_wg", *args, budget, ops.stream())
    else:
        ops.encoder_fwd(imgs_d, flats, outs, acts, H, W, 0 if path == "generic_f32" else 1)
    torch.cuda.synchronize()
    return outs, acts


def _saved_raw(act, n, H, W, stored_bf16):
    """The five saved activations of one problem as device tensors (n, ...) in the format they are stored in."""
    from tacorl_amd import ops

    offs, tot = ops.encoder_act_layout(n, H, W)
    shapes = [(n, oh, ow, c) for (oh, ow), c in zip(R.conv_out(H, W), (32, 64, 64))] + [(n, 128), (n, 256)]
    out = {}
    for j, (stage, shp) in enumerate(zip(STAGES, shapes)):
        seg = act[offs[j]: offs[j + 1] if j + 1 < 5 else tot]
        numel = int(torch.tensor(shp).prod())
        if stored_bf16 and j < 2:  # bf16 at the start of the fp32-sized slot
            seg = seg.view(torch.bfloat16)
        out[stage] = seg[:numel].view(*shp)
    return out


def _saved(act, n, H, W, stored_bf16):
    raw = _saved_raw(act, n, H, W, stored_bf16)
    return {s: (R.nchw(t) if t.dim() == 4 else t.double().cpu()) for s, t in raw.items()}


# ============================================================================================ C1 / C2 / C3
@GEOMS
@pytest.mark.parametrize("path", ["fused", "generic_bf16", "generic_f32"])
def test_forward_layer_by_layer_and_per_image(H, W, path):
    """C1 (fused: encoder_fused.hip, 150 x 200: encoder_ring.hip), C2 (tacorl_encoder_fwd, bf16 and f32 MFMA, fp32 saved
    activations; f32: no operand rounding in the reference) and C3 (bf16 paths)."""
    from oracle import tacorl_oracle as O

    dev = _dev()
    counts = R.fwd_counts(H, W)
    refs = [R.fwd_reference(H, W, i) for i in range(len(counts))]
    flats, packed = _upload([r[0] for r in refs], dev)
    outs, acts = _forward(path, H, W, flats, packed, _images([r[1] for r in refs], dev, path))
    rounded, stored_bf16 = path != "generic_f32", path == "fused"
    level, per_geometry = R.e2e_level(O)
    worst, sa_px, bad = {}, [0.0, 0.0, 0.0, 0.0], []
    e2e = 0.0
    for i, (P, img, ref) in enumerate(refs):
        got = _saved(acts[i], counts[i], H, W, stored_bf16)
        got["out"] = outs[i].double().cpu()
        for stage, sref, bound, info in R.stage_checks(P, img, got, rounded=rounded, stored_bf16=stored_bf16):
            use = R.bound_use(got[stage], sref, bound)
            worst[stage] = max(worst.get(stage, 0.0), use)
            if stage == "sa":
                err = float((got["sa"] - sref).abs().max())
                if err >= sa_px[0]:
                    sa_px = [err, float(bound.max()), info["torch32"], info["floor"]]
            if not use <= 1.0:
                bad.append((f"problem {i}", stage, use))
        if rounded:
            e = R.per_image_relerr(got["out"], ref["out"])
            e2e = max(e2e, float(e.max()))
            if not float(e.max()) <= R.E2E_FACTOR * level:
                bad.append((f"problem {i}", "per-image output", int(e.argmax()), float(e.max())))
    tag = f"{H}x{W} {path}"
    print(f"{tag}: err / bound per stage " + ", ".join(f"{s} {u:.3g}" for s, u in worst.items())
          + f"; soft-argmax {sa_px[0]:.2e} px (bound {sa_px[1]:.2e} = max(4 x torch fp32 {sa_px[2]:.2e}, floor {sa_px[3]:.2e}))"
          + (f"; worst image {e2e:.2e} (bound {R.E2E_FACTOR * level:.2e}, oracle here {per_geometry[(H, W)]:.2e})" if rounded else ""))
    for s, u in worst.items():
        record_margin(f"{tag} {s}", u, 1.0, kind="C1 err / bound")
    record_margin(f"{tag} px", sa_px[0], sa_px[1], floor=sa_px[2], kind="C1 soft-argmax")
    record_margin(f"{tag} px", sa_px[3], sa_px[1], kind="C1 soft-argmax floor")
    if rounded:
        record_margin(tag, e2e, R.E2E_FACTOR * level, floor=per_geometry[(H, W)], kind="C3 per image")
    assert not bad, bad


# ==================================================================================================== C4
@GEOMS
def test_forward_same_image_same_bits_wherever_it_is_served(H, W):
    """One image at positions 0, 15, 16 and last of a problem (both sides of an FC chunk of 16, the ragged tail) and in a
    second problem of the same launch with the same weights: its output row and every saved activation are bit-identical,
    whichever workgroup served it - also on 3 and on 100 workgroups (tacorl_encoder_fwd_fused_wg)."""
    dev = _dev()
    counts = R.fwd_counts(H, W)
    P, img0, _ = R.fwd_reference(H, W, 0)
    img1 = R.fwd_reference(H, W, 1)[1]
    probe = img0[3]
    places = [(0, 0), (0, 15), (0, 16), (0, counts[0] - 1), (1, counts[1] // 2)]
    a, b = img0.clone(), img1.clone()
    for p, k in places:
        (a, b)[p][k] = probe
    flats, packed = _upload([P], dev)
    imgs_d = _images([a, b], dev, "fused")
    first, bad = None, []
    for budget in (None, 3, 100):
        outs, acts = _forward("fused", H, W, flats * 2, packed * 2, imgs_d, budget)
        raw = [_saved_raw(acts[p], counts[p], H, W, True) for p in range(2)]
        assert all(torch.isfinite(o).all() for o in outs)
        for p, k in places:
            here = {"out": outs[p][k], **{s: raw[p][s][k] for s in STAGES}}
            if first is None:
                first = {s: t.clone() for s, t in here.items()}
                assert all(torch.isfinite(t.float()).all() for t in first.values())
            bad += [(budget, p, k, s, int((here[s] != first[s]).sum())) for s in here if not torch.equal(here[s], first[s])]
    assert not bad, bad


# ==================================================================================================== C5
@GEOMS
@pytest.mark.parametrize("path", ["fused", "generic_bf16"])
def test_forward_sharp_softmax(H, W, path):
    """T_SHARP: the largest logit is ~ 100, past exp's fp32 range - the soft-argmax must subtract the maximum (the
    whole-image kernel, the online merge of the deferred pixel and of encoder_ring.hip, softargmax_fwd_kernel)."""
    dev = _dev()
    counts = R.fwd_counts(H, W)
    refs = [R.fwd_reference(H, W, i, R.T_SHARP) for i in range(len(counts))]
    flats, packed = _upload([r[0] for r in refs], dev)
    outs, acts = _forward(path, H, W, flats, packed, _images([r[1] for r in refs], dev, path))
    worst, bad = [0.0, 0.0, 0.0, 0.0, 0.0], []
    for i, (P, img, ref) in enumerate(refs):
        got = _saved(acts[i], counts[i], H, W, path == "fused")
        if not (torch.isfinite(outs[i]).all() and all(torch.isfinite(t).all() for t in got.values())):
            bad.append((f"problem {i}", "not finite"))
        (_, sref, bound, info), = R.stage_checks(P, img, got, stages=("sa",))
        err, use = float((got["sa"] - sref).abs().max()), R.bound_use(got["sa"], sref, bound)
        if use >= worst[0]:
            worst = [use, err, float(bound.max()), info["torch32"], info["floor"]]
        if not use <= 1.0:
            bad.append((f"problem {i}", "sa", use))
    logit = max(float(r[2]["y3"].max()) for r in refs) / R.T_SHARP
    print(f"{H}x{W} {path} T_SHARP (max logit {logit:.0f}): soft-argmax {worst[1]:.2e} px, bound {worst[2]:.2e} = "
          f"max(4 x torch fp32 {worst[3]:.2e}, floor {worst[4]:.2e})")
    record_margin(f"{H}x{W} {path} px", worst[1], worst[2], floor=worst[3], kind="C5 soft-argmax")
    record_margin(f"{H}x{W} {path} px", worst[4], worst[2], kind="C5 soft-argmax floor")
    assert logit > 88.8
    assert not bad, bad


# ==================================================================================================== D1
def _temperature_floors(O, H, W, rounded):
    """golden_util.gradient_floor per problem, as tests/test_kernels_gpu.py:test_encoder_fused_backward: the temperature
    gradient is one global (dp - <p, dp>) cancellation, its reproducibility under 1-ulp weight changes is a floor."""
    key = (H, W, rounded)
    if key not in _floors:
        fl = []
        for i in range(len(R.bwd_counts(H, W))):
            P, img, d_out = R.bwd_problem(H, W, i)
            with O.operand_rounding(torch.bfloat16 if rounded else None):
                def regrad(Pp, img=img, d_out=d_out):
                    Pp = {k: v.detach().requires_grad_(True) for k, v in Pp.items()}
                    return dict(zip(Pp, torch.autograd.grad((O.encoder_fwd(Pp, "", img) * d_out).sum(), list(Pp.values()))))

                fl.append(gradient_floor(regrad, P, regrad(P)).get("model.6.temperature", 0.0))
        _floors[key] = fl
    return _floors[key]


def _backward_setup(H, W, path, problems, dev):
    """Upload, run the path's forward with saved activations -> (flats, imgs_d, acts, d_outs on the device)."""
    Ps, seen, flats, packed = [], {}, [], []
    for P in (p[0] for p in problems):  # problems that share a parameter dict share its device copy
        if id(P) not in seen:
            seen[id(P)] = len(Ps)
            Ps.append(P)
    uf, up = _upload(Ps, dev)
    for p in problems:
        flats.append(uf[seen[id(p[0])]])
        packed.append(up[seen[id(p[0])]])
    imgs_d = _images([p[1] for p in problems], dev, path)
    _, acts = _forward(path, H, W, flats, packed, imgs_d)
    return flats, imgs_d, acts, [p[2].to(dev) for p in problems]


def _named(flat):
    from tacorl_amd import blocks

    return {k: v.detach().double().cpu() for k, v in blocks.encoder_views(flat).items()}


@GEOMS
@pytest.mark.parametrize("path", ["fused", "generic_bf16", "generic_f32"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_backward_against_fp64_by_slice(H, W, path, accumulate):
    """Every gradient per output channel, the conv weights also per kernel tap: the relative error of the slice (floored
    denominators: encoder_ref.slice_relerr) against encoder_ref.backward at GRAD_FACTOR x the fp32 oracle's autograd on the
    same slices, per tensor class over every geometry (encoder_ref.grad_levels); the temperature at least FLOOR_FACTOR x
    its reproducibility floor.  A ReLU gate that fp32 cannot decide (pre-activation within the C1 bound of zero) is taken
    from the forward that fed the backward; a gate that fp32 can decide must be the reference's.  fused: the
    LDS-resident backward fed the fused forward's saved activations; generic: tacorl_encoder_bwd after tacorl_encoder_fwd."""
    from oracle import tacorl_oracle as O
    from tacorl_amd import ops

    dev = _dev()
    rounded = path != "generic_f32"
    probs = R.bwd_reference(O, H, W, rounded=rounded)[0]
    levels, per_geometry = R.grad_levels(O, rounded)
    floors = _temperature_floors(O, H, W, rounded)
    flats, imgs_d, acts, d_outs = _backward_setup(H, W, path, probs, dev)
    if accumulate:
        bases = [R.accumulate_base(f.numel(), 150 + i).to(dev) for i, f in enumerate(flats)]
    else:
        bases = [torch.full_like(f, float("nan")) for f in flats]
    grads = [b.clone() for b in bases]
    ops.encoder_bwd(imgs_d, flats, acts, d_outs, grads, H, W, 0 if path == "generic_f32" else 1, accumulate=accumulate,
                    fused=path == "fused")
    torch.cuda.synchronize()
    worst, bad, gates = {}, [], []
    for i, (P, img, d_out, _, _) in enumerate(probs):
        got = _named(grads[i])
        # the reference under the gates of the forward that fed this backward, where fp32 cannot decide them
        info = {}
        g64 = R.backward(P, img, d_out, rounded=rounded, kernel_acts=_saved(acts[i], img.shape[0], H, W, path == "fused"), info=info)
        gates.append(info["gates"])
        if any(g[2] for g in info["gates"]):
            bad.append((f"problem {i}", "a gate that fp32 can decide differs from the reference's", info["gates"]))
        extra = {}
        if accumulate:
            base = _named(bases[i])
            got = {k: got[k] - base[k] for k in got}
            extra = R.accumulate_rounding(base, g64)
        if not all(torch.isfinite(v).all() for v in got.values()):
            bad.append((f"problem {i}", "not finite"))
            continue
        for (name, kind), e in R.grad_errors(got, g64).items():
            c = R.grad_class(name, kind)
            bound = R.GRAD_FACTOR * levels[c]
            if c == "temperature":
                bound = max(bound, R.FLOOR_FACTOR * floors[i])
            bound += extra.get((name, kind), 0.0)
            if c not in worst or e / bound > worst[c][0] / worst[c][1]:
                worst[c] = (e, bound, per_geometry[(H, W)][c], name)
            if not e <= bound:
                bad.append((f"problem {i}", name, kind, e, bound))
    tag = f"{H}x{W} {path} accumulate={int(accumulate)}"
    print(f"{tag}: worst slice per class, err / bound (oracle's level at this geometry): "
          + ", ".join(f"{c} {e:.2e} / {b:.2e} ({lv:.2e}, {n})" for c, (e, b, lv, n) in worst.items())
          + f"; gates per conv (undecidable at fp32, of those the kernel's decision adopted, decidable but different): {gates}")
    for c, (e, b, lv, n) in worst.items():
        record_margin(f"{tag} {c}", e, b, floor=lv, kind="D1 gradient slices")
    assert not bad, bad


# ==================================================================================================== D2
@GEOMS
@pytest.mark.parametrize("path", ["fused", "generic_bf16"])
def test_backward_is_additive_over_images(H, W, path):
    """Problems A u B, A and B in one launch under the same weights: grad(A u B) = grad(A) + grad(B) element by element up
    to the a-priori bound of the fp32 sums, C_SUM n 2^-24 sum|terms| (n terms per element: images x output pixels) - every
    image's contribution is the same bits in both, only the order of the sum differs.  No reference enters but the scale
    sum|terms|.  An image served twice, a stale double buffer or a slab left out of the reduce breaks it
    (tests/test_encoder_ref_cpu.py: 2e4 x the bound)."""
    from tacorl_amd import ops

    dev = _dev()
    P, img, d_out, g64, terms, na = R.union_reference(H, W)
    problems = [(P, img, d_out), (P, img[:na], d_out[:na]), (P, img[na:], d_out[na:])]
    flats, imgs_d, acts, d_outs = _backward_setup(H, W, path, problems, dev)
    grads = [torch.full_like(f, float("nan")) for f in flats]
    ops.encoder_bwd(imgs_d, flats, acts, d_outs, grads, H, W, 1, fused=path == "fused")
    torch.cuda.synchronize()
    u, a, b = (_named(g) for g in grads)
    worst, bad = (0.0, ""), []
    for name in R.NAMES:
        t, n = terms[name]
        use = R.bound_use(u[name], a[name] + b[name], R.C_SUM * n * R.U32 * t.reshape(u[name].shape))
        worst = max(worst, (use, name))
        if not use <= 1.0:
            bad.append((name, use))
    print(f"{H}x{W} {path}: |grad(A u B) - grad(A) - grad(B)| / bound, worst element: {worst[0]:.3g} ({worst[1]})")
    record_margin(f"{H}x{W} {path} {worst[1]}", worst[0], 1.0, kind="D2 additivity err / bound")
    assert not bad, bad


# ==================================================================================================== D3
class _Fused:
    """The fused backward's entry points on one set of problems, each run into fresh gradient buffers and a fresh,
    identically filled workspace."""

    def __init__(self, H, W, dev):
        from oracle import tacorl_oracle as O
        from tacorl_amd import _lib, ops

        self.H, self.W, self.L, self.ops = H, W, _lib.lib(), ops
        probs = R.bwd_reference(O, H, W)[0]
        self.n = [p[1].shape[0] for p in probs]
        self.flats, self.imgs, self.acts, self.d_outs = _backward_setup(H, W, "fused", probs, dev)
        self.nb = self.L.tacorl_encoder_bwd_fused_ws_bytes(len(self.n), ops.int_array(self.n), H, W)
        assert self.nb > 0

    def buffers(self, accumulate):
        if accumulate:
            grads = [R.accumulate_base(f.numel(), 150 + i).to(f.device) for i, f in enumerate(self.flats)]
        else:
            grads = [torch.full_like(f, float("nan")) for f in self.flats]
        return grads, torch.full((self.nb,), 0x5A, dtype=torch.uint8, device=self.flats[0].device)

    def call(self, name, grads, ws, accumulate=0, prepacked=None, parts=None, ws_bytes=None):
        o = self.ops
        k, n, H, W = len(self.n), o.int_array(self.n), self.H, self.W
        img, par, act, d_out, g = (o.ptr_array(x) for x in (self.imgs, self.flats, self.acts, self.d_outs, grads))
        tail = [o.ptr(ws), self.nb if ws_bytes is None else ws_bytes, o.stream()]
        args = {"tacorl_encoder_bwd_fused": [k, img, par, act, d_out, g, n, H, W, accumulate],
                "tacorl_encoder_bwd_fused_pack": [k, par, n, H, W],
                "tacorl_encoder_bwd_fused_head": [k, par, act, d_out, n, H, W, prepacked],
                "tacorl_encoder_bwd_fused_fc_wgrad": [k, act, d_out, g, n, H, W, accumulate],
                "tacorl_encoder_bwd_fused_conv": [k, img, par, act, g, n, H, W, accumulate, prepacked],
                "tacorl_encoder_bwd_fused_conv_parts": [k, img, par, act, g, n, H, W, accumulate, prepacked, parts]}[name]
        return getattr(self.L, name)(*args, *tail)


def _same_bits(got, want):
    from tacorl_amd import blocks

    bad = {}
    for i, (a, b) in enumerate(zip(got, want)):
        va, vb = blocks.encoder_views(a), blocks.encoder_views(b)
        assert all(torch.isfinite(v).all() for v in vb.values()), i
        bad.update({(i, k): int((va[k] != vb[k]).sum()) for k in va if not torch.equal(va[k], vb[k])})
    return bad


@GEOMS
@pytest.mark.parametrize("accumulate", [0, 1])
def test_backward_engine_entry_points_equal_the_composite(H, W, accumulate, monkeypatch):
    """What the training steps run - _pack, then _head(prepacked = 1) -> _conv(prepacked = 1) and _fc_wgrad - and the
    partial-mask sequence of _conv_parts (parts 1, 2, 4, 8, 16, 32, 64 in dependency order), each on one stream, against
    the composite tacorl_encoder_bwd_fused: the same kernels in a fixed reduction order without atomics, so bit for bit
    (the parts never run the single-launch conv3 stage: their composite runs under TACORL_EBW_FUSE3=0)."""
    F = _Fused(H, W, _dev())
    g_ref, ws = F.buffers(accumulate)
    assert F.call("tacorl_encoder_bwd_fused", g_ref, ws, accumulate) == 0
    g, ws = F.buffers(accumulate)
    assert F.call("tacorl_encoder_bwd_fused_pack", g, ws) == 0
    assert F.call("tacorl_encoder_bwd_fused_head", g, ws, prepacked=1) == 0
    assert F.call("tacorl_encoder_bwd_fused_conv", g, ws, accumulate, prepacked=1) == 0
    assert F.call("tacorl_encoder_bwd_fused_fc_wgrad", g, ws, accumulate) == 0
    torch.cuda.synchronize()
    bad = _same_bits(g, g_ref)
    assert not bad, ("pack -> head -> conv, fc_wgrad", bad)

    monkeypatch.setenv("TACORL_EBW_FUSE3", "0")
    g_ref, ws = F.buffers(accumulate)
    assert F.call("tacorl_encoder_bwd_fused", g_ref, ws, accumulate) == 0
    monkeypatch.delenv("TACORL_EBW_FUSE3")
    g, ws = F.buffers(accumulate)
    assert F.call("tacorl_encoder_bwd_fused_pack", g, ws) == 0
    assert F.call("tacorl_encoder_bwd_fused_head", g, ws, prepacked=1) == 0
    assert F.call("tacorl_encoder_bwd_fused_fc_wgrad", g, ws, accumulate) == 0
    for part in (1, 2, 4, 8, 16, 32, 64):
        assert F.call("tacorl_encoder_bwd_fused_conv_parts", g, ws, accumulate, prepacked=1, parts=part) == 0, part
    torch.cuda.synchronize()
    bad = _same_bits(g, g_ref)
    assert not bad, ("conv_parts 1, 2, 4, 8, 16, 32, 64", bad)


@pytest.mark.parametrize("H,W", [(84, 84), (150, 200)])
def test_backward_refusals_come_before_any_launch(H, W):
    """A partial conv_parts call without prepacked fragments is TACORL_EINVAL (it would re-pack the W^T fragments behind a
    dgrad that reads them), a workspace one byte short is TACORL_ENOMEM - and neither has written a byte of the gradients
    or of the workspace (parts = 1 | 2: the soft-argmax backward of the same call must not have run either)."""
    F = _Fused(H, W, _dev())
    g, ws = F.buffers(0)
    g0, ws0 = [x.clone() for x in g], ws.clone()
    for parts in (2, 1 | 2, 8 | 16, 127 - 64):
        assert F.call("tacorl_encoder_bwd_fused_conv_parts", g, ws, 0, prepacked=0, parts=parts) == EINVAL, parts
    short = {"tacorl_encoder_bwd_fused": {}, "tacorl_encoder_bwd_fused_pack": {}, "tacorl_encoder_bwd_fused_head": dict(prepacked=0),
             "tacorl_encoder_bwd_fused_fc_wgrad": {}, "tacorl_encoder_bwd_fused_conv": dict(prepacked=0),
             "tacorl_encoder_bwd_fused_conv_parts": dict(prepacked=1, parts=1)}
    for name, kw in short.items():
        assert F.call(name, g, ws, ws_bytes=F.nb - 1, **kw) == ENOMEM, name
    torch.cuda.synchronize()
    assert torch.equal(ws, ws0)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g, g0))
