"""The training steps with `device_noise_seed`: after every step each noise buffer of the engine / module is what the NumPy
restatement gives for (seed, step, draw id); a twin without a seed that is fed those tensors through `noise=` logs the same
scalars and ends on the same parameters; a run resumed from a checkpoint draws the noise of the straight run bit for bit; a
module without a seed writes no new checkpoint key.

Tolerance of the twin and resume comparisons: the one with which the step reproduces itself over two runs on one injected
tape.  Measured on the parent commit for the four configurations below (two modules, two steps, the goldens' tapes): every
logged scalar and every parameter bit-identical - so the tolerance is ZERO (profiles/device_noise.md)."""
import pytest
import torch

from tests import device_noise_util as U
from tests.test_step_gpu import to_dev

pytestmark = pytest.mark.gpu


def _shape(mod, batch):
    eng = getattr(mod, "engine", None)
    B = eng.B if eng is not None else mod.noise["eps_plan"].shape[0]
    T = mod.pr._shape[1] if getattr(mod, "_pr_train", False) else None
    return B, T


def _step(mod, batch, noise=None):
    mod.logged = {}
    mod.training_step(to_dev(batch, mod.device), noise=noise)
    torch.cuda.synchronize()


def _same(a, b, what):
    (pa, la), (pb, lb) = a, b
    bad = [f"param {k}" for k in pa if not torch.equal(pa[k], pb[k])]
    bad += [f"log {k}: {la[k]!r} vs {lb.get(k)!r}" for k in la if la[k] != lb.get(k)]
    assert la and not bad, f"{what}: " + "; ".join(bad[:12])


@pytest.mark.parametrize("name", U.CASES)
def test_buffers_are_the_restatement_and_the_taped_twin_agrees(name):
    bs = U.batches(name, 2, B=4 if name == "cql_q" else None)
    mod, twin = U.build(name), U.build(name, seed=None)
    assert twin.__dict__.get("_device_noise") is None and getattr(twin, "engine", twin).__dict__.get("device_noise") is None
    for step, batch in enumerate(bs):
        assert mod._device_noise.state() == {"seed": U.SEED, "step": step}
        _step(mod, batch)
        B, T = _shape(mod, batch)
        bufs = U.check_buffers(mod, B, U.SEED, step)
        if name == "playlmp_dropout":
            assert sum(k.startswith("dropout_") for k in bufs) == 9
        if name == "cql_q":
            assert B == 4 and mod.engine.n == 2 and {"g_pi", "g_cur", "u_rand"} <= set(bufs)
        _step(twin, batch, noise=U.as_tape(mod, bufs, B, T))
        _same(U.snapshot(mod), U.snapshot(twin), f"{name} step {step}: seeded vs taped twin")
    assert mod._device_noise.step == 2
    # a validation step draws too (and moves nothing): the counter advances once
    mod.validation_step(to_dev(bs[0], mod.device))
    torch.cuda.synchronize()
    assert mod._device_noise.step == 3


@pytest.mark.parametrize("name", U.CASES)
def test_resume_draws_the_straight_runs_noise(name, tmp_path):
    from tacorl_amd.lightning import MiniTrainer

    bs = U.batches(name, 4, B=4 if name == "cql_q" else None)
    straight, noise = U.build(name), {}
    MiniTrainer()._attach(straight)
    for step, batch in enumerate(bs):
        _step(straight, batch)
        noise[step] = U.check_buffers(straight, *_shape(straight, batch)[:1], U.SEED, step)
    first = U.build(name)
    ta = MiniTrainer()
    ta._attach(first)
    for batch in bs[:2]:
        _step(first, batch)
    path = str(tmp_path / "last.ckpt")
    ta.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck[first.DEVICE_NOISE_KEY] == {"seed": U.SEED, "step": 2}
    assert set(ck["state_dict"]) == set(first.state_dict()) and not any("noise" in k for k in ck["state_dict"])
    del first
    resumed = U.build(name, seed=U.SEED + 1)  # (the checkpoint's seed and step replace the constructor's)
    tb = MiniTrainer()
    tb._attach(resumed)
    tb.load_checkpoint(path)
    assert resumed._device_noise.state() == {"seed": U.SEED, "step": 2}
    for step in (2, 3):
        _step(resumed, bs[step])
        got = {k: v.detach().clone() for k, (v, *_) in U.noise_buffers(resumed).items()}
        assert set(got) == set(noise[step]) and all(torch.equal(got[k], noise[step][k]) for k in got), f"noise of step {step}"
    _same(U.snapshot(straight), U.snapshot(resumed), f"{name}: straight vs resumed")


def test_unseeded_module_writes_no_checkpoint_key(tmp_path):
    from tacorl_amd.lightning import MiniTrainer

    mod = U.build("cql_q", seed=None)
    tr = MiniTrainer()
    tr._attach(mod)
    ck = tr.dump_checkpoint()
    assert mod.DEVICE_NOISE_KEY not in ck
    assert set(ck) == {"epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers", "hyper_parameters"}
    mod.set_device_noise(5, step=9)
    assert tr.dump_checkpoint()[mod.DEVICE_NOISE_KEY] == {"seed": 5, "step": 9}
