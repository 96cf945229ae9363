"""ActionDecoderLogistic (tacorl_amd/networks/action_decoder.py) as a module on the GPU: forward, loss and BPTT of every
route the module chooses between by shape, against the plain-torch restatement of tests/action_decoder_util.py
(tests/test_action_decoder_cpu.py ties that restatement to the oracle and to central differences) - f32 against fp64 autograd,
bf16 against the restatement with the MFMA's operand rounding - route against route, the twin pass, the bookkeeping of the
bf16 weight mirrors and of the shape-keyed buffers, act() against forward(), and the entry points of the wavefront BPTT and of
its helpers on their own.  Every case asserts WHICH route ran, from the module's own predicates and a log of the entry points
it called; the expected routes are written down from the dispatch code (action_decoder.py forward / backward, rnn_ops.hip
rnn_fwd_batch / tacorl_rnn_linear_bwd_batch / launch_small), not derived by running it."""
import ctypes as C

import pytest
import torch

from tests.action_decoder_util import (TIE_CAP, decoder_loss, flat, is_forward, make_inputs, make_params, rounded_floor)
from tests.golden_util import record_margin

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16 = 0, 1
# fp32 kernel rule (tests/test_seq_gpu.py) and module rule (test_seq_gpu.py / test_birnn_gpu.py):
#   |got - ref64| <= rtol * (|s| + median|s|) + K_REF32 * |ref32 - ref64|
RTOL, RTOL_MODULE, K_REF32 = 1e-5, 1e-4, 4.0
# relative norms against the bf16-rounded restatement (tests/test_kernels_gpu.py), and route against route on the same bf16
# operands (test_action_decoder_heads_dgrad_ring); each is raised to 3 x the reference's own reproducibility floor
# (action_decoder_util.rounded_floor; the factor is test_encoder_fused_backward's) where that is larger
FWD_BF16_ROUNDED, GRAD_BF16_ROUNDED, PATH_VS_PATH = 2e-3, 1e-2, 2e-5
# bf16: ReLU decisions of the module that differ from the rounded restatement's AWAY from an fp32 tie.  In f32 there are
# none (strict).  In bf16 the two sides round their hidden states to bf16 separately: where the fp32 values - a few ulp
# apart - straddle a bf16 boundary, one operand of the next contraction moves by a bf16 ulp (2^-8 relative) and that step's
# pre-activations by ~|w h| 2^-8 ~ 1e-4, above the tie width (1e-4 of mean|z| ~ 5e-5), so a gate whose |z| is that small may
# differ.  Nor does it end there: from that step on the two sides' states of that batch row are ~1e-4 apart instead of
# ~1e-7, each of their elements then straddles a boundary with probability ~1e-4 / 2^-8 ~ 3 %, and the difference is carried
# through the row's later steps and into the layer above.  The count is therefore no product of small independent
# probabilities (that estimate, ~4e-6 of the gates, is ten times below what occurs) but a few first events per case, each
# with a tail: on the CPU the restatement alone, re-evaluated under the floor's 1-ulp weight perturbations, differs from
# itself in 0 gates at most shapes, 1 gate of layer 1 at (37, 5), (1, 9) gates of layers (0, 1) at (832, 3), (1, 3) at
# H = 384, (1, 1) at H = 192 (profiles/action_decoder_module_margins.md has them beside the module's).  That figure - per layer, the worst of the floor's runs (action_decoder_util.rounded_floor) - is the yardstick:
# the module may differ from the restatement in at most GATE_DISAGREE times as many gates as the restatement differs from
# itself, and in none where it does not (the factor is the one the floor carries everywhere in this file).
GATE_DISAGREE = 3


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(name, got, ref, ref32=None, rtol=RTOL_MODULE, scale=None, Tm=None, sparse=False):
    """The elementwise rule above.  scale: magnitudes s other than |ref| (a sum's terms); Tm: rows are sequence-major
    (t*B + b) and the median is taken per time step (test_birnn_gpu._check(T=...): the input gradient shrinks through every
    step of the ReLU-RNN); sparse: the median floored at 1e-3 of the largest magnitude (ReLU-sparse tensors, as there)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    mag = (ref if scale is None else scale.detach().double().cpu()).abs()
    if Tm is not None:
        m3 = mag.view(Tm, -1, mag.shape[-1])
        med = m3.reshape(Tm, -1).median(dim=1).values.view(Tm, 1, 1).expand_as(m3).reshape(mag.shape)
    else:
        med = mag.flatten().median() if mag.numel() else mag.sum()
        if sparse:
            med = torch.maximum(med, 1e-3 * mag.max())
    tol = rtol * (mag + med)
    if ref32 is not None:
        tol = tol + K_REF32 * (ref32.detach().double().cpu() - ref).abs()
    err = (got - ref).abs()
    worst = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"tolerance-use {name}: {worst:.3g}")
    record_margin(name, worst, 1.0, kind="f32 tolerance-use")
    return [] if worst <= 1.0 else [f"{name}: worst error {worst:.3g} x its tolerance (max abs error {err.max().item():.3g})"]


class Calls:
    """The entry points the module calls, in order, with their arguments (a thin wrapper around the module's `call`)."""

    def __init__(self, monkeypatch):
        import tacorl_amd.networks.action_decoder as M

        self.log, real = [], M.call

        def call(name, *args):
            self.log.append((name, args))
            return real(name, *args)

        monkeypatch.setattr(M, "call", call)

    def take(self):
        log, self.log = self.log, []
        return log


@pytest.fixture
def calls(monkeypatch):
    return Calls(monkeypatch)


def _count(log, name):
    return sum(1 for n, _ in log if n == name)


def _ring_tiles(log):
    """(tile, stages) of every ring-GEMM wavefront launch in the log, by the dispatch rules of rnn_ops.hip (rnn_fwd_batch,
    tacorl_rnn_linear_bwd_batch, launch_small), as {"fwd": [...], "bwd": [...]} with one (nprob, tile) per launch.
    THE LIMIT OF THIS: the library does not report the tile it launched, so this is the test's own copy of those rules applied
    to the (nprob, M, M2, N) the module really passed.  What the tile assertions establish is that each case's shape REACHES
    the rule it is here for as the rules stand today - so that the numerical comparison of that case exercises that tile -
    and they fail when the module changes what it passes.  They do not fail when a rule in rnn_ops.hip changes: whoever
    changes one must change this copy and look at ROUTES again."""
    def small(nprob, M, N):
        MT, NTX = (M + 63) // 64, (N // 32 + 7) // 8
        return "64x32/4" if 8 * MT * NTX * nprob <= 192 else "64x32/2"

    out = {"fwd": [], "bwd": []}
    for name, a in log:
        if name in ("tacorl_rnn_linear_fwd_batch_ext", "tacorl_rnn_linear_fwd_batch_twin"):
            nprob, M, M2, N = a[0], a[12] + a[13], a[13], a[15]
        elif name == "tacorl_rnn_linear_fwd_batch":
            nprob, M, M2, N = a[0], a[8], 0, a[10]
        elif name == "tacorl_rnn_linear_bwd_batch":
            nprob, M, M2, N = a[0], a[8], 0, a[10]
        else:
            continue
        if nprob <= 2 and M % 64 == 0:
            tile = small(nprob, M, N)
        elif name != "tacorl_rnn_linear_bwd_batch" and M2 > 0 and nprob > 2 and M >= 512 and M % 128 == 0 and N % 128 == 0:
            tile = "128x128/2"
        elif M % 128 == 0 and N % 64 == 0:
            tile = "128x64/2"
        else:
            tile = small(nprob, M, N)
        out["bwd" if name == "tacorl_rnn_linear_bwd_batch" else "fwd"].append((nprob, tile))
    return out


def _module(H, P, E, L, W):
    from tacorl_amd.networks.action_decoder import ActionDecoderLogistic

    ad = ActionDecoderLogistic(_dev(), state_dim=E, latent_plan_dim=P, hidden_size=H, out_features=7, num_layers=L)
    with torch.no_grad():
        for k, v in ad.blk.views.items():
            v.copy_(W[k])
    return ad


def _case(B, Tm, H, P, E, L, seed):
    """Weights and inputs of a case: CPU tensors and the device copies in the module's layouts."""
    dev = _dev()
    W = make_params(H, P + E, L, seed)
    plan, emb, acts = make_inputs(B, Tm, P, E, seed + 1)
    d = dict(plan=plan.to(dev), emb=emb.reshape(B * (Tm + 1), E).contiguous().to(dev), acts=acts.contiguous().to(dev))
    return W, (plan, emb[:, :Tm], acts[:, :Tm]), d


def _run(ad, d, B, Tm, compute, fwd=None, bwd=None):
    """forward + loss + backward with every output NaN-prefilled (an unwritten element fails the comparison); the results in
    the restatement's form (action_decoder_util.decoder_loss)."""
    from tacorl_amd import ops

    T, E, H = Tm + 1, d["emb"].shape[1], ad.hidden
    ad._ensure(B, Tm)
    ad.heads.fill_(NAN)
    ad.blk.grad.fill_(NAN)
    if getattr(ad, "_bshape", None) == (B, Tm):
        for t in [ad.dx_seq] + ad.dHs + ad.DZ:
            t.fill_(NAN)
    loss = torch.full((2,), NAN, device=ad.dev)  # (loss, gripper accuracy)
    ad.forward(d["plan"], d["emb"], E, B, T, Tm, compute, **(fwd or {}))
    ad.loss(d["acts"], ops.ptr(loss), B, T, Tm, want_grad=True)
    ad.backward(B, Tm, compute, need_input_grad=True, **(bwd or {}))
    torch.cuda.synchronize()
    return {"loss": loss[0].cpu(), "heads": ad.heads[:, :ad.NH].cpu(), "h": [h.view(Tm, B, H).cpu() for h in ad.h],
            "dx_seq": ad.dx_seq.cpu().clone(), "grads": {k: v.detach().cpu().clone() for k, v in ad.blk.grad_views.items()}}


def _gates(got):
    return [h > 0 for h in got["h"]]


# ================================================================================== f32 against fp64
@pytest.mark.parametrize("B,Tm,H,P,E,L", [(5, 6, 128, 16, 32, 2), (37, 5, 35, 14, 32, 2), (64, 3, 256, 16, 32, 3),
                                           (16, 1, 128, 16, 32, 2), (8, 4, 128, 16, 32, 1)])
def test_action_decoder_f32_vs_fp64(B, Tm, H, P, E, L):
    """The f32 path (generic GEMMs, step by step): loss, heads, every layer's hidden states, the input gradient and every
    parameter gradient by reference name against fp64 autograd of the restatement, which takes the module's ReLU decisions
    at ties only (a decision that differs elsewhere raises).  H = 35 / P + E = 46: odd widths, the scalar loaders of the
    generic weight gradient; Tm = 1: the recurrent matrices' gradients are exactly zero."""
    W, ref_in, d = _case(B, Tm, H, P, E, L, seed=B + Tm + H)
    ad = _module(H, P, E, L, W)
    got = _run(ad, d, B, Tm, F32)
    assert not ad._bwd_fast(B, F32)
    r64 = decoder_loss(W, *ref_in, torch.float64, L=L, gates=_gates(got))
    r32 = decoder_loss(W, *ref_in, torch.float32, L=L, gates=_gates(got))
    assert max(r64["ties"]) <= TIE_CAP and max(r32["ties"]) <= TIE_CAP, (r64["ties"], r32["ties"])
    tag = f"f32 B{B}/Tm{Tm}/H{H}/K{P + E}/L{L}"
    g, a, b = flat(got), flat(r64), flat(r32)
    bad = []
    for k in a:
        bad += _check(f"{tag} {k}", g[k], a[k], b[k], Tm=Tm if k == "dx_seq" else None, sparse=k != "dx_seq")
    for l in range(L):
        assert torch.equal(got["grads"][f"rnn.bias_hh_l{l}"], got["grads"][f"rnn.bias_ih_l{l}"])
        if Tm == 1:
            assert float(got["grads"][f"rnn.weight_hh_l{l}"].abs().max()) == 0.0
    assert not bad, "\n".join(bad)


# ================================================================================== bf16 against the rounded restatement
_REFS = {}


def _rounded_ref(key, W, ref_in, L, gates):
    """The bf16-rounded restatement with the module's decisions at ties, and its floor (memoised per case)."""
    ref = decoder_loss(W, *ref_in, torch.float32, L=L, gates=gates, strict=False, rounded=True)
    if key not in _REFS:
        own = decoder_loss(W, *ref_in, torch.float32, L=L, rounded=True)
        _REFS[key] = rounded_floor(W, *ref_in, L, own)
    return ref, _REFS[key]


def _compare_bf16(tag, got, ref, floor, fwd_c=FWD_BF16_ROUNDED, grad_c=GRAD_BF16_ROUNDED, kind="bf16 vs rounded restatement"):
    g, r, bad = flat(got), flat(ref), []
    for k in r:
        assert torch.isfinite(g[k]).all(), f"{tag} {k}: non-finite"
        if float(r[k].double().norm()) == 0.0:
            assert float(g[k].abs().max()) == 0.0, f"{tag} {k}: must be exactly zero"
            continue
        e, fl = _relerr(g[k], r[k]), floor.get(k, 0.0)
        bound = max(fwd_c if is_forward(k) else grad_c, 3 * fl)
        print(f"{kind} {tag} {k}: err {e:.3g} floor {fl:.3g} bound {bound:.3g}")
        record_margin(f"{tag} {k}", e, bound, floor=fl, kind=kind)
        if not e <= bound:
            bad.append(f"{tag} {k}: relative error {e:.3g} > {bound:.3g} (floor {fl:.3g})")
    return bad


# (B, Tm, H, P, E, L) -> what the dispatch code takes there.  Keys: fast (the ring-GEMM path), ext (layer 0's projection as a K
# extension of the ring step: tacorl_rnn_linear_fwd_batch_ext), proj ("bf16": the input rows only; "generic": a projection
# GEMM), square (tacorl_rnn_wgrad_batch), rnn_wgrad / linear_wgrad / bwd_step (calls of the per-matrix ring weight gradient,
# the generic one, the per-step BPTT launch), fwd / bwd: ring tiles that must occur among the wavefront launches.
ROUTES = {
    # ragged rows: 64x32 tiles with the row mask, fused projection + K extension; heads slabbed, every RNN matrix generic
    (5, 6, 128, 16, 32, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=0, linear_wgrad=4, fwd={(3, "64x32/4")}, bwd={(3, "64x32/4")}),
    (37, 5, 128, 16, 32, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=0, linear_wgrad=4, fwd={(3, "64x32/4")}, bwd={(3, "64x32/4")}),
    # (Tm-1) B = 64 but Tm B = 80: W_hh through tacorl_rnn_wgrad, W_ih through the generic kernel
    (16, 5, 128, 16, 32, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=2, linear_wgrad=2),
    # every row count a multiple of 64: one launch for the square matrices; 3-problem launches on small tiles (Tm = 4: the
    # BPTT wavefront holds three problems only from four steps on)
    (64, 4, 128, 16, 32, 2): dict(fast=True, ext=True, square=True, rnn_wgrad=0, linear_wgrad=1, fwd={(3, "64x32/4")}, bwd={(3, "64x32/4")}),
    # M % 128 == 0: 128x64 tiles for the 3-problem launches, forward and backward
    (128, 4, 128, 16, 32, 2): dict(fast=True, ext=True, square=True, rnn_wgrad=0, linear_wgrad=1, fwd={(3, "128x64/2")}, bwd={(3, "128x64/2")}),
    # P + E = 96 (two cameras + a 32-wide plan): K extension without the fused-projection gate.  (B = 32, Tm = 4: 96 and 128
    # rows - W_ih_l1 through tacorl_rnn_wgrad, both W_hh generic)
    (32, 4, 128, 32, 64, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=1, linear_wgrad=3),
    # P + E = 44: ring projection with a width that is no multiple of 8
    (32, 4, 128, 12, 32, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=1, linear_wgrad=3),
    # P + E = 160 > 128: a projection GEMM of its own, plain batched ring steps
    (32, 4, 128, 32, 128, 2): dict(fast=True, ext=False, proj="generic", square=False, rnn_wgrad=1, linear_wgrad=3),
    # three layers: per-step BPTT (2L - 1 > 4), layer-by-layer weight gradients
    (64, 3, 128, 16, 32, 3): dict(fast=True, ext=True, square=False, rnn_wgrad=5, linear_wgrad=1, bwd_step=6),
    # ... and five problems in one forward launch (steps of three layers, projections of two): cut into 4 + 1
    (8, 5, 128, 16, 32, 3): dict(fast=True, ext=True, square=False, rnn_wgrad=0, linear_wgrad=6, bwd_step=12),
    (64, 3, 128, 16, 32, 1): dict(fast=True, ext=True, square=False, rnn_wgrad=1, linear_wgrad=1),
    # Tm = 1 on the fast path: no BPTT launch at all, W_hh gradients zeroed
    (64, 1, 128, 16, 32, 2): dict(fast=True, ext=True, square=False, rnn_wgrad=0, linear_wgrad=2),
    # more than 192 small-tile workgroups: the 2-stage ring
    (832, 3, 128, 16, 32, 2): dict(fast=True, ext=True, square=True, rnn_wgrad=0, linear_wgrad=1, fwd={(3, "64x32/2")}, bwd={(2, "64x32/2")}),
    # N = 384: two N tiles per XCD in the workgroup map
    (64, 3, 384, 16, 32, 2): dict(fast=True, ext=True, square=True, rnn_wgrad=0, linear_wgrad=1),
    # H = 192: not the ring path; the generic GEMMs with bf16 operands
    (8, 5, 192, 16, 32, 2): dict(fast=False),
}


@pytest.mark.parametrize("B,Tm,H,P,E,L", sorted(ROUTES))
def test_action_decoder_bf16_vs_rounded_restatement(B, Tm, H, P, E, L, calls):
    """bf16: the same quantities as relative norms against the restatement under operand_rounding(bf16) (the module's ReLU
    decisions at ties; away from ties they may differ as often as GATE_DISAGREE allows), each within max(project constant,
    3 x the restatement's own floor); the route the case is here for is asserted from the module's predicates and the entry points it called (ROUTES)."""
    from tacorl_amd import ops

    want = ROUTES[(B, Tm, H, P, E, L)]
    W, ref_in, d = _case(B, Tm, H, P, E, L, seed=2 * B + Tm + H + P)
    ad = _module(H, P, E, L, W)
    got = _run(ad, d, B, Tm, BF16)
    log, R, K = calls.take(), B * Tm, P + E
    names = [n for n, _ in log]
    # ---- the route
    assert ad._bwd_fast(B, BF16) == want["fast"]
    if not want["fast"]:
        assert not any(n.startswith("tacorl_rnn_") for n in names) and getattr(ad, "d_heads_b", None) is None
        assert _count(log, "tacorl_linear_wgrad") == 2 * L + 1 and "tacorl_build_ad_input" in names
    else:
        assert ad._heads_ring(R) and ad.d_heads_b is not None and ad.d_heads_b.shape == ((R + 63) // 64 * 64, 256)
        assert _count(log, "tacorl_rnn_wgrad_slabs") == 1, "the heads' weight gradient: row slabs through the ring kernel"
        assert ("tacorl_rnn_linear_fwd_batch_ext" in names) == want["ext"] == (ad._ring_proj() and ad._mirror_ring)
        if want["ext"]:
            assert "tacorl_build_ad_input_bf16" in names and "tacorl_ad_input_proj" not in names and "tacorl_rnn_linear_fwd_batch" not in names
            assert (32 <= K <= 64 and K % 8 == 0) or K in (44, 96)
        else:
            assert want["proj"] == "generic" and "tacorl_rnn_linear_fwd_batch" in names and "tacorl_linear_add_fwd" in names
        n_fwd = sum(_count(log, n) for n in ("tacorl_rnn_linear_fwd_batch_ext", "tacorl_rnn_linear_fwd_batch"))
        cut = sum(1 for s in range(Tm + 2 * (L - 1))
                  if sum(0 <= s - 2 * l < Tm for l in range(L)) + sum(0 <= s - 2 * l + 1 < Tm for l in range(1, L)) > 4)  # (RNN_MAXP)
        assert n_fwd == Tm + 2 * (L - 1) + cut and (cut > 0) == ((B, Tm, L) == (8, 5, 3))
        assert (_count(log, "tacorl_rnn_wgrad_batch") == 1) == want["square"]
        assert _count(log, "tacorl_rnn_wgrad") == want["rnn_wgrad"] and _count(log, "tacorl_linear_wgrad") == want["linear_wgrad"]
        assert _count(log, "tacorl_rnn_linear_bwd_step") == want.get("bwd_step", 0)
        wave = Tm > 1 and 2 * L - 1 <= 4
        # (one launch for the heads' input gradient, then the wavefront's)
        assert _count(log, "tacorl_rnn_linear_bwd_batch") == 1 + (Tm - 1 + 2 * (L - 1) if wave else 0)
        tiles = _ring_tiles(log)
        assert want.get("fwd", set()) <= set(tiles["fwd"]), tiles["fwd"]
        assert want.get("bwd", set()) <= set(tiles["bwd"]), tiles["bwd"]
        if (B, Tm) == (5, 6) or (B, Tm) == (37, 5):
            assert {t for _, t in tiles["fwd"] + tiles["bwd"]} == {"64x32/4"}
        if H == 384:  # 12 N tiles of 32 columns: two per XCD in the workgroup map of every wavefront launch (NTX = 2)
            waves = [a for n, a in log if n in ("tacorl_rnn_linear_fwd_batch_ext", "tacorl_rnn_linear_bwd_batch")]
            ns = {a[15] if len(a) > 12 else a[10] for a in waves}
            assert ns == {384} and (384 // 32 + 7) // 8 == 2
    # ---- the numbers
    key = (B, Tm, H, P, E, L)
    ref, floor = _rounded_ref(key, W, ref_in, L, _gates(got))
    assert max(ref["ties"]) <= TIE_CAP, ref["ties"]
    tag = f"B{B}/Tm{Tm}/H{H}/K{K}/L{L}"
    for l, (mine, own) in enumerate(zip(ref["disagree"], floor["gate disagreement"])):
        print(f"bf16 {tag}: ReLU decisions of layer {l} that differ away from a tie: share {mine:.3g}, the restatement's own {own:.3g}")
        record_margin(f"{tag} layer {l}", mine, GATE_DISAGREE * own, floor=own, kind="bf16 gate disagreement")
        assert mine <= GATE_DISAGREE * own, (l, mine, own)
    bad = _compare_bf16(tag, got, ref, floor)
    for l in range(L):
        assert torch.equal(got["grads"][f"rnn.bias_hh_l{l}"], got["grads"][f"rnn.bias_ih_l{l}"])
    assert not bad, "\n".join(bad)
    assert ops.BF16 == BF16 and ops.F32 == F32


# ================================================================================== twin pass
@pytest.mark.parametrize("B", [256, 5])
def test_action_decoder_twin_pass(B, calls):
    """A second, logging-only plan riding in the launches of forward() (twin rows): its heads equal a plain forward of that
    plan on a fresh module with the same weights, and the real pass - heads, loss, every gradient - is what it is without
    the twin.  B = 256: 512 rows in three-problem launches take the 128x128 tile (the plain pass: 128x64), so the two sides
    may differ in fp32 summation order (the route-against-route bound); B = 5: the same tile on both sides, bit-identical."""
    Tm, H, P, E, L = 4, 128, 16, 32, 2
    W, ref_in, d = _case(B, Tm, H, P, E, L, seed=B + 9)
    plan2 = torch.randn(B, P, generator=torch.Generator().manual_seed(B + 10))
    d2 = dict(d, plan=plan2.to(_dev()))
    alone, second = _module(H, P, E, L, W), _module(H, P, E, L, W)
    ref_real = _run(alone, d, B, Tm, BF16)
    tiles_alone = set(_ring_tiles(calls.take())["fwd"])
    ref_twin = _run(second, d2, B, Tm, BF16)
    calls.take()
    ad = _module(H, P, E, L, W)
    assert ad.twin_ok(B, BF16)
    tw = ad.twin_input_proj(d2["plan"], d["emb"], E, B, Tm + 1, Tm)
    tw.heads.fill_(NAN)
    got = _run(ad, d, B, Tm, BF16, fwd=dict(twin=tw))
    ad.twin_heads(tw, B, Tm)
    torch.cuda.synchronize()
    log = calls.take()
    tiles = set(_ring_tiles(log)["fwd"])
    assert all(a[13] == B for n, a in log if n == "tacorl_rnn_linear_fwd_batch_ext"), "twin rows in every launch"
    assert ((3, "128x128/2") in tiles) == (B == 256) and ((3, "128x64/2") in tiles_alone) == (B == 256)
    twin_heads = tw.heads[:, :ad.NH].cpu()
    assert torch.isfinite(twin_heads).all()
    if tiles == tiles_alone:
        assert torch.equal(twin_heads, ref_twin["heads"])
        for k, v in flat(ref_real).items():
            assert torch.equal(flat(got)[k], v), k
        return
    own = decoder_loss(W, *ref_in, torch.float32, L=L, rounded=True)
    floor = rounded_floor(W, *ref_in, L, own, key=("twin", B))
    ref_in2 = (plan2,) + tuple(ref_in[1:])  # (the twin's heads: the floor of the plan they were computed from)
    floor2 = rounded_floor(W, *ref_in2, L, decoder_loss(W, *ref_in2, torch.float32, L=L, rounded=True), key=("twin2", B))
    e = _relerr(twin_heads, ref_twin["heads"])
    print(f"twin B{B} heads: err {e:.3g} floor {floor2['heads']:.3g}")
    record_margin(f"twin B{B} twin heads", e, max(PATH_VS_PATH, 3 * floor2["heads"]), floor=floor2["heads"], kind="route vs route")
    assert e <= max(PATH_VS_PATH, 3 * floor2["heads"]), e
    bad = _compare_bf16(f"twin B{B}", got, ref_real, floor, PATH_VS_PATH, PATH_VS_PATH, kind="route vs route")
    assert not bad, "\n".join(bad)


# ================================================================================== route against route
@pytest.mark.parametrize("B", [64, 37])
def test_action_decoder_route_vs_route(B, calls):
    """bf16, the same operands on both sides, fp32 summation order apart: the default route against each alternative the
    module's switches select (per-step BPTT, layer-by-layer weight gradients, generic heads weight / input gradient, the
    projection launch of its own), every quantity within max(2e-5, 3 x floor); a prepared backward, the weight gradients on a
    side stream and a second run of the same route are bit-identical to the default."""
    Tm, H, P, E, L = 4, 128, 16, 32, 2
    W, ref_in, d = _case(B, Tm, H, P, E, L, seed=B + 20)
    base_ad = _module(H, P, E, L, W)
    base = _run(base_ad, d, B, Tm, BF16)
    base_log = calls.take()
    own = decoder_loss(W, *ref_in, torch.float32, L=L, rounded=True)
    floor = rounded_floor(W, *ref_in, L, own, key=("rvr", B))
    # what each switch must change in the list of entry points (B = 64; at B = 37 no row count is a multiple of 64 and the
    # weight gradients are generic either way)
    variants = [("bptt_wavefront", dict(attr=("bptt_wavefront", False)), "tacorl_rnn_linear_bwd_step", True),
                ("wavefront=False", dict(bwd=dict(wavefront=False)), "tacorl_rnn_linear_bwd_step", True),
                ("wgrad_batched", dict(attr=("wgrad_batched", False)), "tacorl_rnn_wgrad_batch", False),
                ("heads_wgrad_slabs", dict(attr=("heads_wgrad_slabs", False)), "tacorl_rnn_wgrad_slabs", False),
                ("heads_dgrad_ring", dict(attr=("heads_dgrad_ring", False)), "tacorl_linear_dgrad_splitk", True),
                ("fused_input_proj", dict(attr=("fused_input_proj", False)), "tacorl_ad_input_proj", False)]
    assert _count(base_log, "tacorl_rnn_linear_bwd_step") == 0 and _count(base_log, "tacorl_rnn_wgrad_slabs") == 1
    assert (_count(base_log, "tacorl_rnn_wgrad_batch") == 1) == (B == 64) and _count(base_log, "tacorl_ad_input_proj") == 0
    bad = []
    for tag, how, entry, appears in variants:
        ad = _module(H, P, E, L, W)
        if "attr" in how:
            setattr(ad, *how["attr"])
        got = _run(ad, d, B, Tm, BF16, bwd=how.get("bwd"))
        log = calls.take()
        if tag == "fused_input_proj":
            # (the gate of the fused projection also closes the ring's K extension: a generic projection GEMM, plain ring steps)
            assert "tacorl_rnn_linear_fwd_batch_ext" not in [n for n, _ in log] and _count(log, "tacorl_rnn_linear_fwd_batch") == Tm + 2
        elif tag == "wgrad_batched" and B != 64:
            assert _count(log, entry) == 0
        elif tag == "heads_dgrad_ring":
            assert _count(log, entry) > _count(base_log, entry) and _count(log, "tacorl_rnn_wgrad_slabs") == 0
        else:
            assert (_count(log, entry) > 0) == appears, (tag, entry)
        bad += _compare_bf16(f"B{B} {tag}", got, base, floor, PATH_VS_PATH, PATH_VS_PATH, kind="route vs route")
    # ---- bit-identical repeats
    same = {}
    ad = _module(H, P, E, L, W)
    same["a second run"] = (_run(ad, d, B, Tm, BF16), _run(ad, d, B, Tm, BF16))[1]
    ad = _module(H, P, E, L, W)
    assert ad.prepare_backward(B, Tm, BF16)
    same["prepared=True"] = _run(ad, d, B, Tm, BF16, bwd=dict(prepared=True))
    ad = _module(H, P, E, L, W)
    side = torch.cuda.Stream()
    same["wgrad_stream"] = _run(ad, d, B, Tm, BF16, bwd=dict(wgrad_stream=side))
    for tag, got in same.items():
        for k, v in flat(base).items():
            if not torch.equal(flat(got)[k], v):
                bad.append(f"B{B} {tag}: {k} is not bit-identical to the default run (relative difference {_relerr(flat(got)[k], v):.3g})")
    assert not bad, "\n".join(bad)


# ================================================================================== bookkeeping: mirrors, shapes
def _heads(ad, d, B, Tm, **kw):
    ad._ensure(B, Tm)
    ad.heads.fill_(NAN)
    ad.forward(d["plan"], d["emb"], d["emb"].shape[1], B, Tm + 1, Tm, BF16, **kw)
    torch.cuda.synchronize()
    return ad.heads[:, :ad.NH].cpu()


def test_action_decoder_frozen_and_current_mirrors():
    """The bf16 weight mirrors of the ring path follow the weights: a frozen decoder refreshes them when the parameter
    block's version counter moved (load_state_dict / copy_) and when a new batch shape has replaced the mirror buffers;
    `mirrors_current` is the caller's word about the mirrors of THIS shape only.  Each forward against a fresh module."""
    Tm, H, P, E, L = 3, 128, 16, 32, 2
    W, _, d16 = _case(16, Tm, H, P, E, L, seed=31)
    _, _, d8 = _case(8, Tm, H, P, E, L, seed=32)
    fresh = lambda Wx, d, B: _heads(_module(H, P, E, L, Wx), d, B, Tm)  # noqa: E731
    ad = _module(H, P, E, L, W)
    assert torch.equal(_heads(ad, d16, 16, Tm, frozen=True), fresh(W, d16, 16))
    assert torch.equal(_heads(ad, d16, 16, Tm, frozen=True), fresh(W, d16, 16))  # (mirrors kept: same version)
    W2 = dict(W)
    W2["rnn.weight_hh_l1"] = W["rnn.weight_hh_l1"] * 0.5
    W2["mean_fc.weight"] = W["mean_fc.weight"] * -1.0
    with torch.no_grad():
        ad.blk.views["rnn.weight_hh_l1"].copy_(W2["rnn.weight_hh_l1"])
        ad.blk.views["mean_fc.weight"].copy_(W2["mean_fc.weight"])
    want = fresh(W2, d16, 16)
    assert not torch.equal(want, fresh(W, d16, 16))
    assert torch.equal(_heads(ad, d16, 16, Tm, frozen=True), want), "a frozen forward ran on stale bf16 mirrors"
    # a new shape allocates new (zero) mirrors: frozen at an unchanged version must still fill them
    assert torch.equal(_heads(ad, d8, 8, Tm, frozen=True), fresh(W2, d8, 8)), "frozen forward after a shape change"
    assert torch.equal(_heads(ad, d16, 16, Tm, frozen=True), want), "frozen forward after a second shape change"
    # mirrors_current: B 16 -> 8 -> 16, the caller's promise made for mirrors that no longer exist
    ad = _module(H, P, E, L, W)
    assert torch.equal(_heads(ad, d16, 16, Tm), fresh(W, d16, 16))
    assert torch.equal(_heads(ad, d16, 16, Tm, mirrors_current=True), fresh(W, d16, 16))
    assert torch.equal(_heads(ad, d8, 8, Tm, mirrors_current=True), fresh(W, d8, 8)), "mirrors_current after a shape change"
    assert torch.equal(_heads(ad, d16, 16, Tm, mirrors_current=True), fresh(W, d16, 16)), "mirrors_current after a second change"
    # ... and kept where it holds: an explicit refresh_mirrors() for this shape, then weights the mirrors do not know
    ad.refresh_mirrors(16, Tm)
    with torch.no_grad():
        ad.blk.views["rnn.weight_hh_l0"].mul_(0.5)
    assert torch.equal(_heads(ad, d16, 16, Tm, mirrors_current=True), fresh(W, d16, 16)), "mirrors_current must not refresh"


def _twin_pass(ad, d, plan2, B, Tm):
    """forward() of d with plan2 riding along as the twin; (the twin's heads, the real pass's heads)."""
    E = d["emb"].shape[1]
    tw = ad.twin_input_proj(plan2, d["emb"], E, B, Tm + 1, Tm)
    tw.heads.fill_(NAN)
    ad.heads.fill_(NAN)
    ad.forward(d["plan"], d["emb"], E, B, Tm + 1, Tm, BF16, twin=tw)
    ad.twin_heads(tw, B, Tm)
    torch.cuda.synchronize()
    return tw.heads[:, :ad.NH].cpu().clone(), ad.heads[:, :ad.NH].cpu().clone()


def test_action_decoder_shape_changes_on_one_module():
    """(64, 3) -> (5, 6) -> (64, 3) on one instance, forward + loss + backward in bf16 and then a forward with a twin pass,
    each bit-identical to a fresh instance: the buffers keyed by shape (_shape, _bshape, _bptt_shape, _hd_shape, the twin
    state's _twin.shape) are all replaced, and the zero pad rows of hb / d_heads_b that the slabbed heads weight gradient
    reads are zero again."""
    H, P, E, L = 128, 16, 32, 2
    W = make_params(H, P + E, L, seed=41)
    ad = _module(H, P, E, L, W)
    for i, (B, Tm) in enumerate([(64, 3), (5, 6), (64, 3), (5, 6)]):
        _, _, d = _case(B, Tm, H, P, E, L, seed=41)
        got = _run(ad, d, B, Tm, BF16)
        ref = _run(_module(H, P, E, L, W), d, B, Tm, BF16)
        for k, v in flat(ref).items():
            assert torch.equal(flat(got)[k], v), (i, B, Tm, k, _relerr(flat(got)[k], v))
        R = B * Tm
        assert not ad.hb[-1][R:].any() and not ad.d_heads_b[R:].any()
        plan2 = d["plan"].flip(0).contiguous()
        assert ad.twin_ok(B, BF16)
        twin, real = _twin_pass(ad, d, plan2, B, Tm)
        assert ad._twin.shape == (B, Tm) and torch.isfinite(twin).all()
        twin_ref, real_ref = _twin_pass(_module(H, P, E, L, W), d, plan2, B, Tm)
        assert torch.equal(twin, twin_ref) and torch.equal(real, real_ref) and torch.equal(real, ref["heads"]), (i, B, Tm)
        assert not torch.equal(twin, real)


def test_action_decoder_act_vs_forward():
    """f32: Tm calls of act() with injected noise give forward()'s heads row for row (the hidden state carried between the
    calls), `hidden_state` is h_l[Tm - 1], and clear_hidden_state() restarts from the zero state."""
    from oracle import tacorl_oracle as O

    B, Tm, H, P, E, L = 3, 4, 128, 16, 32, 2
    W, (plan, emb, _), d = _case(B, Tm, H, P, E, L, seed=51)
    ad = _module(H, P, E, L, W)
    ad._ensure(B, Tm)
    ad.forward(d["plan"], d["emb"], E, B, Tm + 1, Tm, F32)
    torch.cuda.synchronize()
    heads = ad.heads[:, :ad.NH].cpu().view(Tm, B, -1)
    hs = [h.view(Tm, B, H).cpu() for h in ad.h]
    g = torch.Generator().manual_seed(52)
    ra, rb = torch.rand(Tm, B, 1, 6, 10, generator=g), torch.rand(Tm, B, 1, 6, generator=g)

    def rollout():
        outs = []
        for t in range(Tm):
            a = ad.act(d["plan"], emb[:, t:t + 1].to(ad.dev), noise=(ra[t].to(ad.dev), rb[t].to(ad.dev)), compute=F32)
            torch.cuda.synchronize()
            outs.append((a.cpu(), ad._act_heads[:, :ad.NH].cpu().clone(), ad.hidden_state.cpu().clone()))
        return outs

    for rnd in range(2):
        outs = rollout()
        for t, (a, hd, hn) in enumerate(outs):
            # (same kernels and operands as forward()'s f32 path, one row block at a time: the fp32 rule with no slack)
            bad = _check(f"act round {rnd} step {t} heads", hd, heads[t], rtol=RTOL)
            for l in range(L):
                bad += _check(f"act round {rnd} step {t} h{l}", hn[l], hs[l][t], rtol=RTOL, sparse=True)
            assert not bad, "\n".join(bad)
            DK = 60
            v = lambda x: x.reshape(B, 1, 6, 10)  # noqa: E731
            want = O.logistic_sample(v(hd[:, 2 * DK:3 * DK]), v(hd[:, DK:2 * DK].clamp(min=O.LOG_SIG_MIN)), v(hd[:, :DK]),
                                     hd[:, None, 3 * DK:], ra[t], rb[t])
            assert a.shape == (B, 1, 7) and torch.allclose(a, want, rtol=1e-4, atol=1e-5), (t, a, want)
        assert torch.equal(outs[-1][2], ad.hidden_state.cpu())
        ad.clear_hidden_state()
        assert ad.hidden_state is None


# ================================================================================== entry points on their own
def _bf(t):
    return t.to(torch.bfloat16)


def _guarded(rows, cols, dev, dtype=torch.float32, guard=3):
    """A NaN-filled buffer of rows + 2 guard blocks; the view in use and the whole."""
    whole = torch.full((rows + 2 * guard, cols), NAN, device=dev, dtype=dtype)
    return whole[guard: guard + rows], whole


def _untouched(name, whole, rows, guard=3):
    w = whole.float().cpu()
    assert torch.isnan(w[:guard]).all() and torch.isnan(w[guard + rows:]).all(), f"{name}: written outside its rows"


COMBOS = [("step", True, True, True), ("last projection", False, True, True), ("projection", False, False, False)]


@pytest.mark.parametrize("nprob", [1, 2, 3, 4])
@pytest.mark.parametrize("M,K,N", [(5, 128, 128), (64, 128, 128), (128, 256, 128), (192, 128, 384), (185, 256, 128)])
def test_rnn_linear_bwd_batch(M, K, N, nprob):
    """tacorl_rnn_linear_bwd_batch: nprob problems y = (x Wt^T + addend) * [mask_src > 0] of one shape in one launch, each
    with its own set of optional operands as the wavefront uses them - a recurrent step (addend, mask, bf16 copy), the last
    step's projection (mask and copy, no addend), any other projection (none) - against fp64 on the same bf16 operands
    (fp32 kernel rule over the sum of the products' magnitudes); the bf16 copy is bf16(y) exactly; rows >= M and the guard
    blocks around every output stay untouched.  Shapes: ragged rows / one 64-row tile / 128-row tiles with two k-steps /
    N = 384 (two N tiles per XCD) / the heads' input gradient (R = 37 * 5 rows, K = 182 padded to 256)."""
    from tacorl_amd import _lib, ops

    dev = _dev()
    ld_add = N + 4
    for shift in range(3 if nprob < 3 else 1):
        g = torch.Generator().manual_seed(M + K + N + 10 * nprob + shift)
        P = []
        for p in range(nprob):
            _, has_add, has_mask, has_yb = COMBOS[(p + shift) % 3]
            x, wt = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g) / K ** 0.5)
            add = torch.randn(M, ld_add, generator=g) if has_add else None
            mask = torch.randn(M, N, generator=g) if has_mask else None
            y, y_all = _guarded(M, N, dev)
            yb, yb_all = _guarded(M, N, dev, torch.bfloat16) if has_yb else (None, None)
            P.append(dict(x=x, wt=wt, add=add, mask=mask, y=y, y_all=y_all, yb=yb, yb_all=yb_all,
                          dx=x.to(dev), dwt=wt.to(dev), dadd=None if add is None else add.to(dev),
                          dmask=None if mask is None else mask.to(dev)))
        _lib.call("tacorl_rnn_linear_bwd_batch", nprob, ops.ptr_array([q["dx"] for q in P]), ops.ptr_array([q["dwt"] for q in P]),
                  ops.ptr_array([q["dadd"] for q in P]), ld_add, ops.ptr_array([q["dmask"] for q in P]),
                  ops.ptr_array([q["y"] for q in P]), ops.ptr_array([q["yb"] for q in P]), M, K, N, ops.stream())
        torch.cuda.synchronize()
        bad = []
        for p, q in enumerate(P):
            tag = f"bwd_batch M{M}/K{K}/N{N} nprob {nprob} problem {p} ({COMBOS[(p + shift) % 3][0]})"
            ref = q["x"].double() @ q["wt"].double().T
            r32 = q["x"].float() @ q["wt"].float().T
            mag = q["x"].double().abs() @ q["wt"].double().abs().T
            if q["add"] is not None:
                ref, r32, mag = ref + q["add"][:, :N].double(), r32 + q["add"][:, :N], mag + q["add"][:, :N].double().abs()
            if q["mask"] is not None:
                keep = q["mask"] > 0
                ref, r32, mag = ref * keep, r32 * keep, mag * keep
            bad += _check(tag, q["y"], ref, r32, rtol=RTOL, scale=mag)
            _untouched(tag, q["y_all"], M)
            if q["yb"] is not None:
                assert torch.equal(q["yb"].cpu(), q["y"].cpu().to(torch.bfloat16)), f"{tag}: the bf16 copy is not bf16(y)"
                _untouched(tag + " bf16", q["yb_all"], M)
        assert not bad, "\n".join(bad)


def test_rnn_linear_bwd_batch_refuses():
    """Arguments the launcher must refuse without launching: nprob 0 / 5, K = 64 (below one k-step), N = 48 (no multiple of
    the tile width), an operand 4 bytes off its 16-byte alignment, ld_add % 4 != 0.  The outputs stay untouched."""
    from tacorl_amd import _lib, ops

    dev = _dev()
    M, K, N = 8, 128, 128
    x, wt = torch.zeros(5, M, K, device=dev, dtype=torch.bfloat16), torch.zeros(5, N, K, device=dev, dtype=torch.bfloat16)
    add, mask = torch.zeros(5, M, N + 4, device=dev), torch.ones(5, M, N, device=dev)
    y = torch.full((5, M, N), NAN, device=dev)
    fn = _lib.lib().tacorl_rnn_linear_bwd_batch

    def rc(nprob=2, K=K, N=N, ld_add=N + 4, off=None):
        ptrs = {k: [C.c_void_p(t[p].data_ptr() + (4 if off == k else 0)) for p in range(5)]
                for k, t in dict(x=x, wt=wt, add=add, mask=mask, y=y).items()}
        return fn(nprob, ops.ptr_array(ptrs["x"]), ops.ptr_array(ptrs["wt"]), ops.ptr_array(ptrs["add"]), ld_add,
                  ops.ptr_array(ptrs["mask"]), ops.ptr_array(ptrs["y"]), None, M, K, N, ops.stream())

    for kw in (dict(nprob=0), dict(nprob=5), dict(K=64), dict(N=48), dict(ld_add=N + 2), dict(off="x"), dict(off="wt"),
               dict(off="add"), dict(off="mask"), dict(off="y")):
        assert rc(**kw) != 0, kw
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    assert rc() == 0  # (the same call with nothing wrong is taken)
    torch.cuda.synchronize()
    assert torch.isnan(y[2:]).all() and not y[:2].any()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("K", [46, 48])
@pytest.mark.parametrize("compute", [F32, BF16])
def test_linear_wgrad(compute, K, with_db, accumulate):
    """tacorl_linear_wgrad: dw (+)= dz^T x, db (+)= column sums of dz, two problems of different row counts in one launch,
    x rows wider apart than K (K = 46: the scalar loader; 48: the vector one), onto destinations prefilled with 0.25 (kept
    when accumulating, overwritten otherwise).  f32 against fp64; bf16 against fp32 of the bf16-rounded operands (fp64 as the
    reference, the fp32 evaluation as its own error) - the fp32 kernel rule over the sums of the products' magnitudes."""
    from tacorl_amd import _lib, ops

    dev = _dev()
    Ms, O, ldx, ld_dz = [37, 100], 40, K + 4, 44  # (ldx 50: scalar loads; 52 with K % 4 == 0: vector loads)
    g = torch.Generator().manual_seed(K + 2 * compute)
    xs = [torch.randn(m, ldx, generator=g) for m in Ms]
    dzs = [torch.randn(m, ld_dz, generator=g) for m in Ms]
    dxs, ddzs = [t.to(dev) for t in xs], [t.to(dev) for t in dzs]
    dw = [_guarded(O, K, dev, guard=4) for _ in Ms]  # (4 guard rows: the destination stays 16-byte aligned)
    db = [_guarded(1, O, dev, guard=1) for _ in Ms]
    for v, _ in dw + db:
        v.fill_(0.25)
    nb = _lib.lib().tacorl_linear_wgrad_ws_bytes(2, ops.int_array(Ms), K, O)
    ws = torch.empty(max(256, nb), dtype=torch.uint8, device=dev)
    _lib.call("tacorl_linear_wgrad", 2, ops.ptr_array(dxs), ldx, ops.ptr_array(ddzs), ld_dz, ops.int_array(Ms), K, O,
              ops.ptr_array([v for v, _ in dw]), ops.ptr_array([v for v, _ in db]) if with_db else None, accumulate, compute,
              ops.ptr(ws), ws.numel(), ops.stream())
    torch.cuda.synchronize()
    bad = []
    for p, m in enumerate(Ms):
        x, dz = xs[p][:, :K], dzs[p][:, :O]
        if compute == BF16:
            x, dz = _bf(x).float(), _bf(dz).float()
        base = 0.25 if accumulate else 0.0
        tag = f"linear_wgrad {'bf16' if compute else 'f32'} K{K} db {with_db} acc {accumulate} problem {p}"
        bad += _check(tag + " dw", dw[p][0] - base, dz.double().T @ x.double(), dz.T @ x, rtol=RTOL,
                      scale=dz.double().abs().T @ x.double().abs())
        _untouched(tag + " dw", dw[p][1], O, guard=4)
        if with_db:
            bad += _check(tag + " db", db[p][0][0] - base, dz.double().sum(0), dz.sum(0), rtol=RTOL, scale=dz.double().abs().sum(0))
        else:
            assert torch.equal(db[p][0].cpu(), torch.full((1, O), 0.25)), "db == NULL: nothing may be written"
        _untouched(tag + " db", db[p][1], 1, guard=1)
    assert not bad, "\n".join(bad)


def test_bf16_copy_helpers():
    """tacorl_pad_to_bf16, tacorl_transpose_pad_to_bf16, tacorl_to_bf16_batch: torch.equal against the torch expression, pad
    columns exactly zero, nothing written past the end (NaN guards)."""
    from tacorl_amd import _lib, ops

    dev = _dev()
    g = torch.Generator().manual_seed(61)
    for rows, cols, ld_src, ld_dst in [(37, 182, 192, 256), (128, 44, 44, 128), (1, 1, 5, 8), (300, 48, 48, 128)]:
        src = torch.randn(rows, ld_src, generator=g)
        dsrc, (dst, whole) = src.to(dev), _guarded(rows, ld_dst, dev, torch.bfloat16)
        _lib.call("tacorl_pad_to_bf16", ops.ptr(dsrc), ld_src, ops.ptr(dst), ld_dst, rows, cols, ops.stream())
        torch.cuda.synchronize()
        want = torch.zeros(rows, ld_dst)
        want[:, :cols] = src[:, :cols]
        assert torch.equal(dst.cpu(), _bf(want)), (rows, cols)
        assert not dst[:, cols:].any()
        _untouched("pad_to_bf16", whole, rows)
    for R, Cc, ld_dst in [(182, 128, 256), (33, 32, 64), (1, 96, 32), (64, 64, 64)]:
        src = torch.randn(R, Cc, generator=g)
        dsrc, (dst, whole) = src.to(dev), _guarded(Cc, ld_dst, dev, torch.bfloat16)
        _lib.call("tacorl_transpose_pad_to_bf16", ops.ptr(dsrc), ops.ptr(dst), R, Cc, ld_dst, ops.stream())
        torch.cuda.synchronize()
        want = torch.zeros(Cc, ld_dst)
        want[:, :R] = src.t()
        assert torch.equal(dst.cpu(), _bf(want)), (R, Cc)
        assert not dst[:, R:].any()
        _untouched("transpose_pad_to_bf16", whole, Cc)
    counts = [12, 4100, 20, 128 * 128, 4]  # (12, 4100, 20, 4: no multiples of 8)
    srcs = [torch.randn(c, generator=g) for c in counts]
    dsrc = [s.to(dev) for s in srcs]
    dsts = [_guarded(1, c, dev, torch.bfloat16, guard=1) for c in counts]
    _lib.call("tacorl_to_bf16_batch", len(counts), ops.ptr_array(dsrc), ops.ptr_array([v for v, _ in dsts]),
              (C.c_long * len(counts))(*counts), ops.stream())
    torch.cuda.synchronize()
    for s, (v, whole) in zip(srcs, dsts):
        assert torch.equal(v[0].cpu(), _bf(s)), s.numel()
        _untouched("to_bf16_batch", whole, 1, guard=1)


@pytest.mark.parametrize("P,E", [(12, 32), (16, 32), (32, 64), (64, 64)])
def test_build_ad_input_bf16(P, E):
    """tacorl_build_ad_input_bf16: rows t*B + b = bf16([plan_b | emb_{b,t} | 0 ...]) of 128 columns for t < Tm < T, the
    embeddings' rows wider apart than E; exact, pad columns zero, nothing past the last row."""
    from tacorl_amd import _lib, ops

    dev = _dev()
    B, T, Tm, ld = 5, 4, 3, E + 8
    g = torch.Generator().manual_seed(P + E)
    plan, emb = torch.randn(B, P, generator=g), torch.randn(B * T, ld, generator=g)
    out, whole = _guarded(Tm * B, 128, dev, torch.bfloat16)
    dplan, demb = plan.to(dev), emb.to(dev)
    _lib.call("tacorl_build_ad_input_bf16", ops.ptr(dplan), ops.ptr(demb), ld, ops.ptr(out), B, T, Tm, P, E,
              ops.stream())
    torch.cuda.synchronize()
    want = torch.zeros(Tm, B, 128)
    want[:, :, :P] = plan
    want[:, :, P:P + E] = emb.view(B, T, ld)[:, :Tm, :E].transpose(0, 1)
    assert torch.equal(out.cpu(), _bf(want.view(Tm * B, 128)))
    assert not out[:, P + E:].any()
    _untouched("build_ad_input_bf16", whole, Tm * B)
