"""The d_model-32 plan-recognition launch (tacorl_amd/csrc/pr_fused.hip: pr_encoder_fused_kernel<1|2>) at every edge of its
FFN chunk schedule and of its split over the four waves, through the C entry points, against the fp64 restatement of
tests/pr_ref.py with that module's a-priori bounds (as tests/test_pr_fp64_gpu.py, whose device harness is reused):

  T 16 | 32        one or two row tiles per lane; one (head, query) pair per lane on half of the wave or on the whole of it
  FF 256           one chunk: three waves have none (they request chunk 0, in bounds, and skip the loop)
  FF 1280          five chunks: two rounds for wave 0, one for waves 1 - 3
  FF 2048          eight chunks, two rounds for every wave (the headline step)
  FF 2304          nine chunks: a third round for wave 0, and the FFN1 biases read from global memory (not staged)
  L 1 | 2 | 3      the partial-sum buffer's parity, the shared attention operand rewritten behind the previous layer's barrier
  B 1 | 3, ld_emb 32 | 40

  S  train launch: every saved tensor of every layer per stage (the kernel's own saved input), pooled; NaN-filled outputs
  Q  bit equality where the code promises it: inference == train on every common output (pooled; head, plan of the sample
     launches), two consecutive launches, B = 1 against row 0 of B = 3
  X  the action decoder's bf16 input rows from the sampling launch == tacorl_build_ad_input_bf16 on the same plan and
     embeddings, pad columns included, rows t >= Tm untouched; the refusals of the new arguments

A test collects all its figures before it asserts."""
import ctypes as C

import pytest
import torch

from tests import pr_ref as R
from tests.test_pr_fp64_gpu import EINVAL, NAN, SAVE_KEYS, TAIL, _all_nan, _buf, _Net, _same_bits

pytestmark = pytest.mark.gpu

CASES = [(T, FF, L, ld) for T in (16, 32) for FF in (256, 1280, 2048, 2304) for L in (1, 2, 3) for ld in (32, 40)]
B3 = 3


def _same_run(a, b, rows=slice(None)):
    """Every output of two launches, bit for bit (b's rows `rows` against a)."""
    return (all(_same_bits(a[k], b[k][rows]) for k in ("pooled", "head", "plan") if not _all_nan(b[k]))
            and all(_all_nan(a[k]) == _all_nan(b[k]) for k in ("pooled", "head", "plan"))
            and all(_same_bits(x[k], y[k][rows]) for x, y in zip(a["sv"], b["sv"]) for k in SAVE_KEYS if not _all_nan(y[k]))
            and all(_all_nan(x[k]) == _all_nan(y[k]) for x, y in zip(a["sv"], b["sv"]) for k in SAVE_KEYS))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_FF%d_L%d_ld%d" % c)
def test_chunk_schedule_per_stage_and_bit_equalities(case):
    T, FF, L, ld = case
    P, _ = R.reference(32, T, FF, L, B3, A=16, ld_emb=ld)
    net = _Net(P)
    from tacorl_amd import _lib

    assert _lib.lib().tacorl_pr_encoder_fused_supported(32, T, R.H, FF, L) == 1
    tag = "stream T%d FF%d L%d ld%d" % case
    train, plain, smp, tsmp = (net.launch(m) for m in ("train", "plain", "sample", "train_sample"))
    x0, _ = R.stage_input(P["emb"][..., :32], P["pos"])
    facts = {"bf16 mirror is RNE of the block": net.mirror_ok,
             "guard tails untouched": all(r["tails"] for r in (train, plain, smp, tsmp)),
             "xin[0] == emb + pos bit for bit": _same_bits(train["sv"][0]["xin"], x0),
             "train: head / plan untouched": _all_nan(train["head"]) and _all_nan(train["plan"]),
             "inference: no save written": all(_all_nan(s[k]) for r in (plain, smp) for s in r["sv"] for k in SAVE_KEYS)}
    # ---- S: every stage of every layer on the kernel's own saved input; the inference launch's pooled / head / plan
    use = {}
    for l in range(L):
        sv = {k: train["sv"][l][k].double() for k in SAVE_KEYS}
        for name, ref, bound in R.stage_checks(P, sv, l):
            if name == "y2" and l + 1 < L:
                name, got = f"xin[{l + 1}]", train["sv"][l + 1]["xin"]
            elif name == "y2":
                pref, _ = R.stage_pool(ref)
                use["pooled (inference)"] = R.bound_use(smp["pooled"], pref, R.pool_bound(ref, bound))
                name, got, ref, bound = "pooled", train["pooled"], pref, R.pool_bound(ref, bound)
            else:
                got, name = sv[name], f"{name}[{l}]"
            use[name] = R.bound_use(got, ref, bound)
    A = P["A"]
    Wc, bc = net.Wc[:-TAIL].view(2 * A, 32).cpu(), net.bc[:-TAIL].cpu()
    for name, ref, bound, _e32 in R.head_checks(Wc, bc, smp["pooled"], smp["head"], smp["plan"], P["eps"], P["min_std"],
                                                R.sample_level(32, T)):
        use[f"{name} (inference)"] = R.bound_use(smp[name], ref, bound)
    # ---- Q: bit equalities
    facts["inference pooled == train pooled"] = _same_bits(plain["pooled"], train["pooled"])
    facts["sample == train_sample: pooled, head, plan"] = all(_same_bits(smp[k], tsmp[k]) for k in ("pooled", "head", "plan"))
    facts["sample pooled == plain pooled"] = _same_bits(smp["pooled"], plain["pooled"])
    facts["train_sample saves == train saves"] = all(_same_bits(a[k], b[k]) for a, b in zip(tsmp["sv"], train["sv"])
                                                     for k in SAVE_KEYS)
    facts["second train launch identical"] = _same_run(net.launch("train"), train)
    facts["second sample launch identical"] = _same_run(net.launch("sample"), smp)
    one_t = net.launch("train", emb=P["emb"][:1], eps=P["eps"][:1])
    one_s = net.launch("sample", emb=P["emb"][:1], eps=P["eps"][:1])
    facts["B = 1 == row 0 of B = 3 (train)"] = one_t["tails"] and _same_run(one_t, train, slice(0, 1))
    facts["B = 1 == row 0 of B = 3 (sample)"] = one_s["tails"] and _same_run(one_s, smp, slice(0, 1))
    print(tag, {k: f"{v:.2g}" for k, v in use.items()}, facts)
    assert all(facts.values()), facts
    assert max(use.values()) <= 1.0, {k: v for k, v in use.items() if v > 1.0}


# --------------------------------------------------------------------------------------------------------------- X
ROWS = dict(T=16, Tm=15, P=16, E=32)  # the headline step: latent plan 16, one camera's 32 features, window 16


def _rows_setup(ld_ad):
    from tacorl_amd import _lib

    T, Tm, Pn, E = (ROWS[k] for k in ("T", "Tm", "P", "E"))
    P, _ = R.reference(32, T, 2048, 2, B3, A=Pn)
    net = _Net(P)
    dev = net.dev
    emb = P["emb"].to(dev).contiguous()
    eps = P["eps"].to(dev).contiguous()
    g = torch.Generator().manual_seed(5)
    emb_ad = torch.full((B3 * T, ld_ad), NAN)
    emb_ad[:, :E] = torch.rand(B3 * T, E, generator=g) * 2 - 1
    emb_ad = emb_ad.to(dev)
    pooled, head, plan = _buf(B3 * 32, dev), _buf(B3 * 2 * Pn, dev), _buf(B3 * Pn, dev)
    base = (_lib.ptr(emb), emb.shape[2], _lib.ptr(net.flat), _lib.ptr(net.pb), net.foff, _lib.ptr(pooled), B3, 32, T, R.H, 2048, 2,
            _lib.ptr(net.Wc), _lib.ptr(net.bc), _lib.ptr(eps), _lib.ptr(head), _lib.ptr(plan), Pn, float(P["min_std"]))
    keep = (emb, eps, emb_ad, pooled, head, plan, net)
    return base, keep


@pytest.mark.parametrize("ld_ad", [32, 44])
def test_decoder_input_rows_from_the_sampling_launch(ld_ad):
    from tacorl_amd import _lib

    T, Tm, Pn, E = (ROWS[k] for k in ("T", "Tm", "P", "E"))
    base, keep = _rows_setup(ld_ad)
    emb, eps, emb_ad, pooled, head, plan, net = keep
    dev = net.dev
    nrow = T * B3  # (the buffer has rows for t < T; only t < Tm are written)
    xb = torch.full((nrow * 128 + TAIL,), NAN, device=dev, dtype=torch.bfloat16)
    _lib.call("tacorl_pr_encoder_fused_sample_rows", *base, _lib.ptr(xb), Tm, Pn, E, _lib.ptr(emb_ad), ld_ad, _lib.stream())
    torch.cuda.synchronize()
    got_plan, got_head, got_pooled = plan.clone(), head.clone(), pooled.clone()
    ref = torch.full((nrow * 128 + TAIL,), NAN, device=dev, dtype=torch.bfloat16)
    _lib.call("tacorl_build_ad_input_bf16", _lib.ptr(plan), _lib.ptr(emb_ad), ld_ad, _lib.ptr(ref), B3, T, Tm, Pn, E, _lib.stream())
    pooled.fill_(NAN), head.fill_(NAN), plan.fill_(NAN)
    _lib.call("tacorl_pr_encoder_fused_sample", *base, _lib.stream())
    torch.cuda.synchronize()
    w = Tm * B3 * 128
    bits = lambda t: t.view(torch.int16)  # noqa: E731
    rows = xb[:w].view(Tm, B3, 128).float().cpu()
    facts = {"written rows == tacorl_build_ad_input_bf16, bit for bit": bool(torch.equal(bits(xb[:w]), bits(ref[:w]))),
             "written rows finite (no NaN left in the pad)": bool(torch.isfinite(xb[:w].float()).all()),
             "pad columns zero": bool((rows[..., Pn + E:] == 0).all()),
             "plan columns == bf16(plan)": bool(torch.equal(rows[..., :Pn], got_plan[:-TAIL].view(1, B3, Pn).bfloat16().float().cpu()
                                                            .expand(Tm, B3, Pn))),
             "rows t >= Tm and the guard tail untouched": _all_nan(xb[w:].float()),
             "pooled, head, plan == the launch without the rows": all(
                 _same_bits(a[:-TAIL].cpu(), b[:-TAIL].cpu()) and _all_nan(a[-TAIL:])
                 for a, b in ((got_pooled, pooled), (got_head, head), (got_plan, plan)))}
    print(facts)
    assert all(facts.values()), facts


def test_decoder_input_rows_refusals():
    """Each call returns TACORL_EINVAL and launches nothing: pooled, head, plan and the destination stay NaN."""
    from tacorl_amd import _lib

    T, Tm, Pn, E = (ROWS[k] for k in ("T", "Tm", "P", "E"))
    base, keep = _rows_setup(32)
    emb, eps, emb_ad, pooled, head, plan, net = keep
    xb = torch.full((T * B3 * 128 + TAIL,), NAN, device=net.dev, dtype=torch.bfloat16)
    fn = _lib.lib().tacorl_pr_encoder_fused_sample_rows
    st = _lib.stream()
    off2 = C.c_void_p(xb.data_ptr() + 2)  # (two bytes further: in bounds whatever a launch would do)
    off8 = C.c_void_p(xb.data_ptr() + 8)
    x, e = _lib.ptr(xb), _lib.ptr(emb_ad)
    rcs = {"null destination": fn(*base, None, Tm, Pn, E, e, 32, st),
           "destination + 2 bytes": fn(*base, off2, Tm, Pn, E, e, 32, st),
           "destination + 8 bytes": fn(*base, off8, Tm, Pn, E, e, 32, st),
           "P + E = 129": fn(*base, x, Tm, Pn, 113, e, 128, st),
           "Tm = T + 1": fn(*base, x, T + 1, Pn, E, e, 32, st),
           "Tm = 0": fn(*base, x, 0, Pn, E, e, 32, st),
           "E = 0": fn(*base, x, Tm, Pn, 0, e, 32, st),
           "P != A": fn(*base, x, Tm, 8, E, e, 32, st),
           "null embeddings": fn(*base, x, Tm, Pn, E, None, 32, st),
           "ld_ad < E": fn(*base, x, Tm, Pn, E, e, 28, st)}
    torch.cuda.synchronize()
    wrong = {k: v for k, v in rcs.items() if v != EINVAL}
    assert not wrong, wrong
    assert all(_all_nan(t.float()) for t in (pooled, head, plan, xb)), "a refused call wrote to an output"
