"""Conditions on the encoder's fp64 reference and on the inputs of tests/test_encoder_fp64_gpu.py - nothing here runs a
kernel.  (1) tests/encoder_ref.py restates the oracle: its forward and backward agree with oracle.tacorl_oracle at the fp32
oracle's own accuracy.  (2) The inputs are discriminating: at T_PEAKED the keypoints move from image to image and no two
images' outputs are closer than 2 % of their norm, so a check per image can tell a row from its neighbour.  (3) The bounds
the GPU tests apply (taken from the same module, encoder_ref) are at least 10 x below the local faults they are there to
catch - if a bound has to grow on the GPU, this file says what it stops catching."""
import pytest
import torch

from tests import encoder_ref as R

GEOMS = pytest.mark.parametrize("H,W", R.GEOMETRIES)


@GEOMS
def test_reference_restates_the_oracle(H, W):
    """The level is the fp32 oracle's own accuracy: without operand rounding it differs from the fp64 restatement by fp32
    summation only.  With bf16 operand rounding the two also differ where an fp32 value next to a rounding boundary
    rounds the other way than the fp64 one; one such operand moves by one bf16 ulp, 2^-8 of its value, so no image and no
    gradient slice can be off by more than 2^-8 unless the two do not compute the same thing."""
    from oracle import tacorl_oracle as O

    P, img = R.fwd_problem(H, W, 1)
    e32 = R.per_image_relerr(O.encoder_fwd(P, "", img), R.forward(P, img, rounded=False)["out"])
    with O.operand_rounding(torch.bfloat16):
        er = R.per_image_relerr(O.encoder_fwd(P, "", img), R.forward(P, img)["out"])
    print(f"forward {H}x{W}: fp32 oracle vs fp64, per image: max {e32.max():.2e}; with bf16 operands: median {er.median():.2e} max {er.max():.2e}")
    assert e32.max() < 64 * R.U32            # 257-term sums of fp32: a few ulp
    assert er.median() <= 4 * e32.max()      # most images: no operand rounds differently
    assert er.max() < 2.0 ** -8
    for rounded in (False, True):
        probs, errs = R.bwd_reference(O, H, W, rounded=rounded)
        levels = R.class_levels(errs)
        print(f"backward {H}x{W} rounded={rounded}: fp32 oracle autograd vs fp64, worst slice per class: "
              + ", ".join(f"{k} {v:.2e}" for k, v in levels.items()))
        for c, v in levels.items():
            # (the temperature gradient is one global (dp - <p, dp>) cancellation: golden_util.gradient_floor, not this)
            if c != "temperature":
                assert v < (2.0 ** -8 if rounded else 1e-5), (c, v)
        assert all(torch.isfinite(g).all() for p in probs for g in p[3].values())


@GEOMS
def test_inputs_are_discriminating(H, W):
    for i, n in enumerate(R.fwd_counts(H, W)):
        P, img, r = R.fwd_reference(H, W, i)
        assert torch.equal(img, img.to(torch.bfloat16).float()) and img.abs().max() <= 1  # exact in bf16
        logit = float(r["y3"].max() / R.T_PEAKED)
        assert 4 < logit < 40, logit
        if n > 1:
            sep, spread = R.separation(r["out"]), R.keypoint_spread(r["sa"])
            print(f"{H}x{W} problem {i} ({n} images): max logit {logit:.1f}, separation {sep:.3f}, keypoint spread {spread:.3f} px")
            assert sep >= 0.02, sep
            assert spread >= 0.2, spread
    # the synthetic temperature (~1) makes the same encoder degenerate: that is what the peaked temperature is for
    P1, img = R.fwd_problem(H, W, 0, T=None)
    r1 = R.forward(P1, img)
    assert R.keypoint_spread(r1["sa"]) < 0.05
    # T_SHARP: logits past exp's fp32 range, the reference stays finite
    Ps, img, rs = R.fwd_reference(H, W, 0, R.T_SHARP)
    assert float(rs["y3"].max() / R.T_SHARP) > 88.8
    assert all(torch.isfinite(v).all() for v in rs.values())
    assert float(R.soft_argmax(rs["y3"].float(), torch.tensor(R.T_SHARP)).isfinite().all())


def _faults(n):
    """{name: (stage whose result it corrupts, in-place corruption)}: the local faults a whole-tensor norm dilutes."""
    last = n - 1
    return {
        "last conv1 row of one image zeroed": ("y1", lambda x: x[min(7, last), :, -1, :].zero_()),
        "last conv1 pixel of every image zeroed": ("y1", lambda x: x[:, :, -1, -1].zero_()),
        "one conv1 channel of one image zeroed": ("y1", lambda x: x[0, 31].zero_()),
        "last conv2 column of the last image zeroed": ("y2", lambda x: x[last, :, :, -1].zero_()),
        "one conv3 pixel doubled in every image": ("y3", lambda x: x[:, :, 0, 0].mul_(2)),
        "last image's conv3 output replaced by its neighbour's": ("y3", lambda x: x[last].copy_(x[last - 1])),
    }


@GEOMS
def test_forward_bounds_catch_local_faults(H, W):
    """Every fault against the C1 bound of the stage it corrupts (element by element, reference on the clean input of
    that stage), and its effect on the worst image's output against the C3 bound."""
    from oracle import tacorl_oracle as O

    P, img, r = R.fwd_reference(H, W, 0)
    n = img.shape[0]
    checks = {s: (ref, bound) for s, ref, bound, _ in R.stage_checks(P, img, r)}
    for s, (ref, bound) in checks.items():  # the reference on its own stages: nothing but the stored rounding of y1 / y2
        assert R.bound_use(r[s], ref, bound) <= 1.0, s
    e2e_bound = R.E2E_FACTOR * R.e2e_level(O)[0]
    print(f"{H}x{W}: C3 bound {e2e_bound:.2e} (oracle's worst image {R.e2e_level(O)[0]:.2e}), separation {R.separation(r['out']):.3f}")
    assert R.separation(r["out"]) > 2 * e2e_bound  # a swapped or duplicated image shows in C3
    ratios = {}
    for name, (stage, corrupt) in _faults(n).items():
        def hook(s, t, stage=stage, corrupt=corrupt):
            if s == stage:
                t = t.clone()
                corrupt(t)
            return t
        bad = R.forward(P, img, hook=hook)
        ratios[name] = (R.bound_use(bad[stage], *checks[stage]), float(R.per_image_relerr(bad["out"], r["out"]).max()) / e2e_bound)
    Pd = {k: v.double() for k, v in P.items()}
    w1 = R.bf16(Pd["model.0.weight"]).clone()
    w1[5, 1, 7, 0] = 0
    ratios["one conv1 weight tap zeroed"] = (R.bound_use(R.conv_relu(img.double(), w1, Pd["model.0.bias"], 4), *checks["y1"]), None)
    shifted = img.double().clone()
    shifted[n // 2] = shifted[n // 2].roll(1, dims=1)
    ratios["one image's rows shifted by one"] = (
        R.bound_use(R.conv_relu(shifted, R.bf16(Pd["model.0.weight"]), Pd["model.0.bias"], 4), *checks["y1"]), None)
    for name, (c1, c3) in ratios.items():
        print(f"  {name}: {c1:.3g} x its stage's C1 bound" + ("" if c3 is None else f", worst image {c3:.3g} x the C3 bound"))
        assert c1 >= R.FAULT_RATIO, (name, c1)


def test_backward_bounds_catch_an_image_counted_twice_or_dropped():
    """D1 / D2 at 84 x 84: the gradients with one image counted twice (what a stale double buffer or a work-unit
    partition that serves an image twice gives) and with one image left out, against the additivity bound of D2 (per
    element) and the per-slice bound of D1."""
    from oracle import tacorl_oracle as O

    H, W = 84, 84
    probs, levels = R.bwd_reference(O, H, W)[0], R.grad_levels(O)[0]
    P, img, d_out, g, terms = probs[0]
    one = R.backward(P, img[3:4], d_out[3:4])
    for sign, what in ((1.0, "counted twice"), (-1.0, "dropped")):
        bad = {k: g[k] + sign * one[k] for k in g}
        add = max(R.bound_use(bad[k], g[k], R.C_SUM * terms[k][1] * R.U32 * terms[k][0]) for k in g if "model" in k and "temp" not in k)
        errs = R.grad_errors(bad, g)
        d1 = max(e / (R.GRAD_FACTOR * levels[R.grad_class(*k)]) for k, e in errs.items() if k[0].startswith("model.") and "temp" not in k[0])
        print(f"one image of {img.shape[0]} {what}: {add:.3g} x the D2 bound (worst conv gradient element), {d1:.3g} x the D1 bound (worst conv slice)")
        assert add >= R.FAULT_RATIO and d1 >= R.FAULT_RATIO


def test_an_undecidable_relu_gate_outweighs_the_gradient_bound():
    """Why D1 takes the gates fp32 cannot decide from the kernel's forward: conv1's pre-activation of image 12, channel 22,
    pixel (9, 3) of the second 64 x 64 backward problem is -5.6e-9, 2e-4 of the C1 bound away from zero - a correct fp32 sum
    may land on either side.  Decided the other way it switches one dZ1 element on, and that alone moves the channel's bias
    gradient by 2.7 % and its weight gradient by 1 %: 3 x the D1 bound.  A gate that fp32 CAN decide is never adopted."""
    from oracle import tacorl_oracle as O

    P, img, d_out, g64, _ = R.bwd_reference(O, 64, 64)[0][1]
    r = R.forward(P, img)
    acts = {k: r[k].clone() for k in ("y1", "y2", "y3")}
    info = {}
    g = R.backward(P, img, d_out, kernel_acts=acts, info=info)
    assert all(torch.equal(g[k], g64[k]) for k in g) and all(a == 0 and d == 0 for _, a, d in info["gates"])
    assert info["gates"][0][0] > 0 and r["y1"][12, 22, 9, 3] == 0
    acts["y1"][12, 22, 9, 3] = 1e-9  # the other decision
    g = R.backward(P, img, d_out, kernel_acts=acts, info=info)
    assert info["gates"][0][1:] == (1, 0)
    errs, levels = R.grad_errors(g, g64), R.grad_levels(O)[0]
    print({k: f"{v:.2e}" for k, v in R.class_levels([errs]).items()}, {k: f"{R.GRAD_FACTOR * v:.2e}" for k, v in levels.items()})
    assert errs[("model.0.bias", "channel")] > 2 * R.GRAD_FACTOR * levels["bias"]
    acts["y1"][0, 0, 0, 0] = 0.0 if r["y1"][0, 0, 0, 0] > 0 else 1.0  # a decidable gate
    R.backward(P, img, d_out, kernel_acts=acts, info=info)
    assert info["gates"][0][2] == 1
