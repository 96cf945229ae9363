"""Generate the DR3 fixtures (tests/golden/{cql_dr3,tacorl_dr3,val_cql_dr3}.npz) by running the UNMODIFIED reference on CPU
with `with_dr3=True` (reference modules/cql/cql_offline_lightning.py:424-437, 496-499).

Build container only (needs the reference tree, like oracle/gen_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_dr3_golden.py            # all cases
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_dr3_golden.py cql_dr3

Nothing under oracle/ changes: oracle.ref_harness already forwards `with_dr3` / `dr3_coefficient` overrides to the reference
constructors, and the cases run through oracle.gen_golden.run_case as they are.

The coefficient.  A parity test can only see the term if it is large enough: otherwise it would pass with the term missing.
So, per case, the coefficient starts at the reference default 0.03 and is multiplied by 10 until, at step 0 in the reference,
  (a) |q1_dr3_loss| and |q2_dr3_loss| are >= 1e-2 (below that floor the step tests' scalar check stops being relative), and
  (b) for every conv weight of the q1 and q2 encoders ||g_with - g_without|| / ||g_with|| >= 3e-2 (100 x the step tests'
      gradient tolerance), g_without being the same step of the same module built with with_dr3=False.
Both are asserted on the chosen value, which is written into the fixture's config (overrides.dr3_coefficient) together with
the measured figures (dr3_probe).  The validation case takes its probe from a training step of the same module and batch.
With the synthetic parameters of these cases 0.03 already meets both (terms 0.42 - 0.71, shares 48 - 83 %): the loop is there
in case a change of the cases makes it miss.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gen_golden as G  # noqa: E402
from oracle import ref_harness as H  # noqa: E402
from tacorl_amd import synth  # noqa: E402

CASES = {
    # cql_q's shape: flat CQL baseline, discrete gripper, Q phase
    "cql_dr3": dict(kind="cql", B=3, cams={"rgb_static": (84, 84)}, epoch=5, steps=2, seed=61),
    # tacorl_q's shape with two windows: frozen LMP, no decoder fine-tune, Q phase
    "tacorl_dr3": dict(kind="tacorl", B=2, T=16, cams={"rgb_static": (84, 84)}, latent=16, epoch=5, finetune_ad=False,
                       steps=2, seed=62),
    # validation_step with the term: the same scalars, nothing moves
    "val_cql_dr3": dict(kind="cql", B=3, cams={"rgb_static": (84, 84)}, epoch=5, steps=1, seed=63, validate=True),
}
DR3_FLOOR, GRAD_SHARE = 1e-2, 3e-2
START, MAX_COEF = 0.03, 3e4


def _step0(c, **overrides):
    """One training step of the reference module of case c at its step-0 batch: (logged scalars, {name: gradient as the
    parameter's own optimiser saw it}).  The same construction as oracle.gen_golden.run_case."""
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    cams = c["cams"]
    if c["kind"] == "tacorl":
        lmp = H.build_play_lmp(cams=tuple(sorted(cams)), latent_plan_dim=c["latent"], seq_len=c["T"])
        mod = H.build_tacorl(lmp, finetune_action_decoder=c["finetune_ad"], **overrides)
        batch = synth.make_play_batch(c["seed"] * 100, c["B"], c["T"], cams)
    else:
        mod = H.build_cql(cams=tuple(sorted(cams)), **overrides)
        batch = synth.make_transition_batch(c["seed"] * 100, c["B"], cams)
    synth.fill_params_(mod, c["seed"])
    mod.train()
    mod.current_epoch = c.get("epoch", 0)
    mod.logged, mod.grad_log = {}, []
    with H.record_noise(H.NoiseTape()):
        mod.training_step(batch) if c["kind"] == "tacorl" else mod.training_step(batch, 0)
    order = ["log_alpha", "log_alpha_prime", "actor", "q1", "q2"]
    assert len(mod.grad_log) == len(order), len(mod.grad_log)
    # (a backward leaves gradients on more than its optimiser's group: each group is read from the backward that follows its
    # own zero_grad, as oracle.gen_golden.run_case reads them)
    prefixes = ["actor.", "q1", "q2", "log_alpha_prime", "log_alpha"]  # (log_alpha_prime in front of its prefix log_alpha)
    group = lambda n: next((p.rstrip(".") for p in prefixes if n.startswith(p)), None)  # noqa: E731
    grads = {n: t for g, gl in zip(order, mod.grad_log) for n, t in gl.items() if group(n) == g}
    return {k.split("/", 1)[1]: v for k, v in mod.logged.items()}, grads


def probe(c, coef, without):
    """(smallest |q*_dr3_loss|, smallest share of the term in a critic encoder's conv-weight gradient) at step 0."""
    logs, g = _step0(c, with_dr3=True, dr3_coefficient=coef)
    conv = [n for n, t in g.items() if n.startswith(("q1.encoder.", "q2.encoder.")) and t.dim() == 4]
    assert len(conv) == 2 * 3 * len(c["cams"]), conv
    share = min(((g[n] - without[n]).norm() / g[n].norm()).item() for n in conv)
    return min(abs(logs["q1_dr3_loss"]), abs(logs["q2_dr3_loss"])), share


def choose_coefficient(name, c):
    logs0, without = _step0(c, with_dr3=False)
    assert "q1_dr3_loss" not in logs0
    coef = START
    while True:
        small, share = probe(c, coef, without)
        print(f"[{name}] dr3_coefficient {coef:g}: min |q*_dr3_loss| = {small:.4g}, min conv-gradient share = {share:.4g}")
        if small >= DR3_FLOOR and share >= GRAD_SHARE:
            return coef, small, share
        coef *= 10.0
        assert coef <= MAX_COEF, f"[{name}] no coefficient up to {MAX_COEF:g} makes the term visible"


if __name__ == "__main__":
    which = sys.argv[1:] or list(CASES)
    for n in which:
        c = dict(CASES[n])
        coef, small, share = choose_coefficient(n, c)
        assert small >= DR3_FLOOR and share >= GRAD_SHARE
        c["overrides"] = dict(with_dr3=True, dr3_coefficient=coef)
        c["dr3_probe"] = dict(min_abs_dr3_loss=small, min_conv_grad_share=share)
        G.run_case(n, c)
        size = os.path.getsize(os.path.join(G.OUT, n + ".npz"))
        assert size <= 1 << 20, f"{n}.npz is {size} bytes: over the size limit of a committed fixture"
