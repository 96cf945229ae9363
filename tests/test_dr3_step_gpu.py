"""The whole training / validation step with the DR3 term (with_dr3=True) on the GPU, against the goldens the unmodified
reference produced (tools/gen_dr3_golden.py: cql_dr3, tacorl_dr3, val_cql_dr3).  The modules are built as
tests/test_step_gpu.py builds them, and its tolerances apply: every logged scalar - q{1,2}_dr3_loss and the q{1,2}_loss that
include it among them - at 1e-4, step-0 gradients against the goldens' fingerprints at GRAD_RTOL, parameters after each step
at RTOL / PARAM_ATOL.  The CPU oracle's step knows nothing of DR3, so where full gradient tensors are compared the
restatement is the oracle's gradients plus the term's own, taken by autograd from tests/dr3_ref.py on the oracle's encoder
forward (dr3_ref.golden_terms); parameters after a step are checked against the golden only."""
import copy

import pytest
import torch

from tests import dr3_ref as R
from tests import test_step_gpu as S
from tests.golden_util import Golden, check_stats, gradient_floor, resync_oracle, spec_for

pytestmark = pytest.mark.gpu

DR3_KEYS = ("q1_dr3_loss", "q2_dr3_loss")


def build_cql(g, compute="f32", **over):
    from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

    cams = sorted(g.cams)
    kw = dict(S.CQL_YAML)
    kw.update(g.cfg.get("overrides", {}))
    kw.update(over)
    return CQL_Offline(actor=dict(S.ACTOR, discrete_gripper=True), critic=S.CRITIC, real_world=True, obs_modalities=cams,
                       goal_modalities=cams, action_dim=7, device="cuda:0", compute_dtype=compute, image_dtype=compute, **kw)


def build(g, compute="f32", **over):
    mod = S.build_tacorl(g, compute, **over) if g.cfg["kind"] == "tacorl" else build_cql(g, compute, **over)
    mod.load_state_dict(g.params(), strict=False)
    mod.current_epoch = g.cfg["epoch"]
    return mod


def oracle_spec(g):
    """The oracle's ACSpec of the golden's module: golden_util.spec_for without the two DR3 overrides, which it does not know."""
    g2 = copy.copy(g)
    g2.cfg = dict(g.cfg, overrides={k: v for k, v in g.cfg["overrides"].items() if k not in ("with_dr3", "dr3_coefficient")})
    return spec_for(g2)


def oracle_params(g):
    from oracle import tacorl_oracle as O

    frozen = ("perceptual_encoder.", "plan_recognition.") if g.cfg["kind"] == "tacorl" else ()
    return O.require_grad_(g.params(), frozen_prefixes=frozen)


def restated_step(g, P, opts, spec, step):
    """(logs, plan or None, gradients) of the oracle's step on P with the DR3 term added: its value into q{1,2}_dr3_loss and
    q{1,2}_loss, its gradient onto the critics' encoder gradients.  P is stepped by the oracle (without the term): callers
    resynchronise it from the module before the next step."""
    from oracle import tacorl_oracle as O

    batch, noise, epoch = g.batch(step), g.noise(step), g.cfg["epoch"]
    vals, dgr = R.golden_terms(g, P, step)  # (first: the oracle's step moves P)
    if g.cfg["kind"] == "tacorl":
        logs, plan, grads = O.tacorl_step(P, opts, spec, batch, noise, epoch)
    else:
        (logs, grads), plan = O.cql_step(P, opts, spec, batch, noise, epoch), None
    grads = dict(grads)
    for n, gr in dgr.items():
        grads[n] = grads[n] + gr
    for k, v in vals.items():
        logs[f"{k}_dr3_loss"] = v
        logs[f"{k}_loss"] = logs[f"{k}_loss"] + v
    return logs, plan, grads


def run_step(mod, g, step, validate=False):
    mod.logged = {}
    batch, noise = S.to_dev(g.batch(step), mod.device), S.to_dev(g.noise(step), mod.device)
    fn = mod.validation_step if validate else mod.training_step
    fn(batch, noise=noise) if g.cfg["kind"] == "tacorl" else fn(batch, 0, noise=noise)
    torch.cuda.synchronize()
    return {k.split("/", 1)[1]: v for k, v in mod.logged.items()}


@pytest.mark.parametrize("name", ["cql_dr3", "tacorl_dr3"])
def test_dr3_step_f32(name):
    from oracle import tacorl_oracle as O

    g = Golden(name)
    mod = build(g)
    assert mod.engine.dr3 == g.cfg["overrides"]["dr3_coefficient"]
    spec, P = oracle_spec(g), oracle_params(g)
    opts = O.make_opts(P, spec)
    for step in range(g.cfg["steps"]):
        if step:
            resync_oracle(mod, P, opts)  # see golden_util.resync_oracle
        got = run_step(mod, g, step)
        exp = g.logged(step)
        assert set(DR3_KEYS) <= set(exp) and set(DR3_KEYS) <= set(got)
        print(f"{name} step {step}: " + ", ".join(f"{k} {got[k]:.7g} (reference {exp[k]:.7g})" for k in DR3_KEYS + ("q1_loss", "q2_loss")))
        before, opts0 = S._snap(P), copy.deepcopy(opts)
        ologs, oplan, ograds = restated_step(g, P, opts, spec, step)
        floor = gradient_floor(lambda Pp: restated_step(g, Pp, copy.deepcopy(opts0), spec, step)[2], before, ograds)
        bad = S.check_logs(got, exp)
        bad += [f"restatement {b}" for b in S.check_logs(got, ologs)]
        if oplan is not None and S.relerr(mod.plan, g.latent_plan(step)) > S.RTOL:
            bad.append(f"latent plan relerr {S.relerr(mod.plan, g.latent_plan(step)):.3g}")
        bad += S.compare_with_oracle_grads(mod, ograds, S.GRAD_RTOL, floor)
        if step == 0:
            bad += check_stats(mod.named_gradients(), g.stats(step, "grad"), rtol=S.GRAD_RTOL, what="golden grad ")
        bad += check_stats(mod.state_dict(), g.stats(step, "param"), rtol=S.RTOL, atol=S.PARAM_ATOL, what="golden param ")
        assert not bad, f"step {step}:\n" + "\n".join(bad[:25])


def test_dr3_validation_step():
    """validation_step with the term (val_cql_dr3): the reference's `validation/*` scalars, and nothing moves."""
    g = Golden("val_cql_dr3")
    mod = build(g)
    mod.eval()
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    opt_before = [o.state_dict() for o in S.L_as_list(mod.configure_optimizers())]
    got = run_step(mod, g, 0, validate=True)
    assert mod.logged and all(k.startswith("validation/") for k in mod.logged), sorted(mod.logged)
    exp = g.logged(0)
    assert set(DR3_KEYS) <= set(exp) and set(exp) <= set(got), sorted(set(exp) - set(got))
    bad = S.check_logs(got, exp)
    after = mod.state_dict()
    bad += [f"{k} moved" for k, v in before.items() if not torch.equal(v, after[k])]
    for o0, o in zip(opt_before, S.L_as_list(mod.configure_optimizers())):
        s1 = o.state_dict()["state"]
        for i, st in o0["state"].items():
            if not all(torch.equal(st[f], s1[i][f]) for f in ("step", "exp_avg", "exp_avg_sq")):
                bad.append(f"optimizer {o.name}: state of parameter {i} moved")
    assert not bad, "\n".join(bad[:25])


def test_dr3_tacorl_step_bf16_mode():
    """bf16 compute against the golden, at the tolerances tests/test_step_gpu.py::test_tacorl_step_bf16_mode states for this
    module: the logged losses of the first step 3e-2 relative, the sampled latent plan 2e-2."""
    g = Golden("tacorl_dr3")
    mod = build(g, compute="bf16")
    got = run_step(mod, g, 0)
    exp = g.logged(0)
    print("tacorl_dr3 bf16: " + ", ".join(f"{k} {got[k]:.6g} (reference {exp[k]:.6g})" for k in DR3_KEYS))
    bad = S.check_logs(got, exp, rtol=3e-2)
    e = S.relerr(mod.plan, g.latent_plan(0))
    if e > 2e-2:
        bad.append(f"latent plan relerr {e:.3g}")
    assert not bad, "\n".join(bad)


def restated_params(P_stepped, before, opts0, spec, grads):
    """The parameters after the restated step: the oracle's own step has moved P_stepped WITHOUT the term, which is right
    for everything but the critics, so q1 / q2 are stepped again from `before` - clip, Adam with the optimiser state of
    before the step - on the restated gradients, as the oracle's ac_update steps them."""
    from oracle import tacorl_oracle as O

    after = {k: v for k, v in P_stepped.items()}
    redo = S._snap(before)
    for key in ("q1", "q2"):
        names = O.group_names(redo, key + ".")
        gg = {n: grads[n].clone() for n in names}
        O.clip_grads_(gg, names, spec.clip_grad_val)
        copy.deepcopy(opts0[key]).step(redo, gg)
        after.update({n: redo[n] for n in names})
    return after


@pytest.mark.parametrize("name", ["cql_dr3"])
def test_dr3_step_bf16_vs_rounded_oracle(name):
    """bf16 compute: the comparison and the constants of tests/test_step_gpu.py::test_cql_step_bf16_vs_rounded_oracle and
    ::test_tacorl_step_bf16_vs_rounded_oracle (BF16_LOG_RTOL 2e-3 on the logged scalars, BF16_PLAN_RTOL on the plan,
    BF16_GRAD_RTOL 1e-2 on every gradient or its floor, the step-flip fraction on the post-step parameters) against the
    oracle with the same operand rounding, the DR3 term restated under that rounding too and the critics stepped on the
    restated gradients; two optimiser steps, each from the module's own parameters.  (CQL_Offline only: the same comparison
    on tacorl_dr3 was taken out together with what else this file ran in front of the captured TACORL step when a replay of
    that step crashed in the runtime's graph launch and the cause was not found.)"""
    from oracle import tacorl_oracle as O

    g = Golden(name)
    mod = build(g, compute="bf16")
    spec, P = oracle_spec(g), oracle_params(g)
    opts = O.make_opts(P, spec)
    bad = []
    for step in range(g.cfg["steps"]):
        if step:
            resync_oracle(mod, P, opts)
        before = S._snap(P)
        got = run_step(mod, g, step)
        opts0 = copy.deepcopy(opts)
        with O.operand_rounding(torch.bfloat16):
            ologs, oplan, ograds = restated_step(g, P, opts, spec, step)
            floor = gradient_floor(lambda Pp: restated_step(g, Pp, copy.deepcopy(opts0), spec, step)[2], before, ograds)
        floor = S._with_bf16_sensitivity(floor, ograds, restated_step(g, S._snap(before), copy.deepcopy(opts0), spec, step)[2])
        print(f"{name} bf16 step {step}: " + ", ".join(f"{k} {got[k]:.6g} (rounded restatement {ologs[k]:.6g})" for k in DR3_KEYS))
        after = restated_params(P, before, opts0, spec, ograds)
        plan = (mod.plan, oplan) if oplan is not None else (None, None)
        bad += S._bf16_compare(mod, got, ologs, ograds, before, after, step, *plan, floor=floor)
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("name", ["cql_dr3", "tacorl_dr3"])
def test_dr3_step_eager_and_captured_are_bit_identical(name):
    """The step with the term as eager launches and as the captured graph (first step: warm-up and capture, third: a
    replay): the same logged scalars and the same gradients, bit for bit - the DR3 launch is a node of the graph like its
    neighbours, with no host read and no atomics."""
    g = Golden(name)
    eager, graph = build(g), build(g)
    graph.enable_graph()
    for i, step in enumerate((0, 1, 1)):
        a, b = run_step(eager, g, step), run_step(graph, g, step)
        assert set(DR3_KEYS) <= set(a) and a.keys() == b.keys()
        diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        assert not diff, (i, diff)
        ge, gg = eager.named_gradients(), graph.named_gradients()
        diff = [k for k in ge if not torch.equal(ge[k], gg[k])]
        assert not diff, (i, diff[:10])
    assert len(graph._graphs) == 1


class _CountingLib:
    """Stands in for the loaded library: counts every entry point fetched for a call."""

    def __init__(self, real):
        self.__dict__.update(real=real, counts={})

    def __getattr__(self, name):
        self.counts[name] = self.counts.get(name, 0) + 1
        return getattr(self.real, name)


def count_calls(mod, g, step):
    """{entry point: calls} of one eager training step of mod (buffers allocated and workspaces grown by earlier steps)."""
    from tacorl_amd import _lib

    real = _lib.lib()
    proxy = _CountingLib(real)
    _lib._lib = proxy
    try:
        run_step(mod, g, step)
    finally:
        _lib._lib = real
    return proxy.counts


# Entry-point calls of one eager CQL_Offline.training_step on the golden cql_q (B = 3, one 84 x 84 camera, Q phase, second
# step), counted with count_calls on the commit before DR3: nothing exposes the captured graph's node count, and every
# kernel node of the graph is one of these calls.
PARENT_CALLS = {"f32": 29, "bf16": 77}


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_no_change_without_dr3(compute):
    """with_dr3=False: no dr3 key is logged, the encoder stage has no q*_nx problem and no DR3 buffer, and one eager step
    makes exactly the calls it made before the term existed.  With the term: one DR3 launch and one more copy launch."""
    g = Golden("cql_q")
    off, on = build(g, compute), build(g, compute, with_dr3=True, dr3_coefficient=0.03)
    counts = {}
    for key, mod in (("off", off), ("on", on)):
        run_step(mod, g, 0)
        counts[key] = count_calls(mod, g, 1)
        logged = {k.split("/", 1)[1] for k in mod.logged}
        assert (set(DR3_KEYS) <= logged) == (key == "on") and (not set(DR3_KEYS) & logged) == (key == "off"), sorted(logged)
    e = off.engine
    assert e.dr3 is None and not hasattr(e, "dr3_in") and not any(k[0].endswith("_nx") and k[0] != "a_nx" for k in e.enc_out)
    assert ("q1_nx", "rgb_static") in on.engine.enc_out and ("q2_nx", "rgb_static") in on.engine.enc_out
    print(f"{compute}: entry-point calls of one eager step without DR3: {sum(counts['off'].values())}, with: {sum(counts['on'].values())}")
    assert "tacorl_dr3_fwd_bwd" not in counts["off"] and counts["on"]["tacorl_dr3_fwd_bwd"] == 1
    assert sum(counts["off"].values()) == PARENT_CALLS[compute], (sum(counts["off"].values()), counts["off"])
    more = {k: v - counts["off"].get(k, 0) for k, v in counts["on"].items() if v != counts["off"].get(k, 0)}
    if compute == "bf16":  # the fused forward takes the two problems into its one launch
        assert more == {"tacorl_dr3_fwd_bwd": 1, "tacorl_copy_cols_batch": 1}, more
