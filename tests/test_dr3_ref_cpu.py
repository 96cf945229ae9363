"""Conditions on the DR3 restatement (tests/dr3_ref.py) and on the constructors - nothing here runs a kernel.
(1) The restatement, applied to the oracle's encoder forward on a golden's parameters and batch, equals the q*_dr3_loss the
unmodified reference logged (tools/gen_dr3_golden.py), at 1e-6 relative.  (2) The bounds the GPU test applies are at least
10 x below what a single dropped row or a single dropped column does at B = 3, and plain fp32 torch stays inside them.
(3) with_dr3=True builds for CQL_Offline and TACORL and reaches the engine; VIB still raises, the D4RL modules still raise."""
import pytest
import torch

from tests import cfg_util as C
from tests import dr3_ref as R
from tests.golden_util import Golden

FAULT_RATIO = 10.0
GOLDENS = ["cql_dr3", "tacorl_dr3", "val_cql_dr3"]


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_equals_the_reference(name):
    g = Golden(name)
    ov = g.cfg["overrides"]
    assert ov["with_dr3"] is True and ov["dr3_coefficient"] > 0
    # the generator's own conditions on the coefficient (a): the term is above check_logs' floor, (b): it is a visible share
    # of every conv-weight gradient of the critics' encoders
    assert g.cfg["dr3_probe"]["min_abs_dr3_loss"] >= 1e-2 and g.cfg["dr3_probe"]["min_conv_grad_share"] >= 3e-2
    exp = g.logged(0)
    with torch.no_grad():
        emb = R.golden_embeddings(g, g.params())
    for k, (eo, en) in emb.items():
        assert eo.shape == (g.cfg["B"], 32 * len(g.cams))
        got = float(R.dr3_loss(eo, en, ov["dr3_coefficient"]))
        ref = exp[f"{k}_dr3_loss"]
        assert abs(ref) >= 1e-2
        assert abs(got - ref) <= 1e-6 * abs(ref), (k, got, ref)
        assert abs(R.value(eo, en, ov["dr3_coefficient"]) - ref) <= 1e-5 * abs(ref)  # the fp64 form, from fp32 embeddings
    # the logged critic losses include the term
    for k in ("q1", "q2"):
        parts = exp[f"bellman_{k}_loss"] + exp[f"conservative_{k}_loss"] + exp[f"{k}_dr3_loss"]
        assert abs(exp[f"{k}_loss"] - parts) <= 1e-5 * abs(parts)


def test_restatement_gradient_is_autograd_of_the_reference_expression():
    p = R.problem(3, 64, 64, 1, n=1)[0]
    obs = p["obs"].double().requires_grad_(True)
    (g,) = torch.autograd.grad(R.dr3_loss(obs, p["next"].double(), R.f32(0.03)), obs)
    assert torch.allclose(g, R.grad_term(p["next"], 0.03, 1.0), rtol=1e-14, atol=0)
    assert torch.allclose(0.5 * g, R.grad_term(p["next"], 0.03, 0.5), rtol=1e-14, atol=0)


@pytest.mark.parametrize("Eo", [32, 64])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_bounds_catch_a_dropped_row_and_a_dropped_column(Eo, gs):
    B, coef = 3, 0.03
    for p in R.problem(B, Eo, Eo + 8, 2):
        obs, nxt, d = p["obs"][:, :Eo], p["next"][:, :Eo], p["d"][:, :Eo]
        v, vb = R.value(obs, nxt, coef), R.value_bound(obs, nxt, coef)
        T, gb = R.grad_term(nxt, coef, gs), R.grad_bound(d, nxt, coef, gs)
        worst_v, worst_g = float("inf"), float("inf")
        for b in range(B):  # row b left out of the sum / of the gradient add
            keep = torch.ones(B, dtype=torch.bool)
            keep[b] = False
            v_bad = float((obs[keep].double() * nxt[keep].double()).sum() * (R.f32(coef) / B))
            worst_v = min(worst_v, abs(v_bad - v) / vb)
            worst_g = min(worst_g, float((T[b].abs() / gb[b]).min()))
        for j in range(Eo):  # column j left out
            keep = torch.ones(Eo, dtype=torch.bool)
            keep[j] = False
            v_bad = float((obs[:, keep].double() * nxt[:, keep].double()).sum() * (R.f32(coef) / B))
            worst_v = min(worst_v, abs(v_bad - v) / vb)
            worst_g = min(worst_g, float((T[:, j].abs() / gb[:, j]).min()))
        print(f"Eo {Eo} gs {gs}: smallest fault / bound: value {worst_v:.3g}, gradient element {worst_g:.3g}")
        assert worst_v >= FAULT_RATIO and worst_g >= FAULT_RATIO
        # overwriting instead of adding is a fault of size |d_before|
        assert float((d.double().abs() / gb).min()) >= FAULT_RATIO


@pytest.mark.parametrize("B", [1, 3, 63, 64, 65, 257])
@pytest.mark.parametrize("Eo", [32, 64])
def test_fp32_torch_stays_inside_the_bounds(B, Eo):
    """No bound is tighter than fp32 can meet: the same arithmetic in plain fp32 torch (its own summation order)."""
    coef, gs = 0.03, 0.5
    for p in R.problem(B, Eo, Eo, 3):
        obs, nxt, d = p["obs"], p["next"], p["d"]
        v32 = float((obs * nxt).sum() * torch.tensor(R.f32(coef) / B, dtype=torch.float32))
        assert abs(v32 - R.value(obs, nxt, coef)) <= R.value_bound(obs, nxt, coef)
        s = torch.tensor(R.f32(coef) * gs / B, dtype=torch.float32)
        d32 = d + s * nxt
        err = (d32.double() - (d.double() + R.grad_term(nxt, coef, gs))).abs()
        assert bool((err <= R.grad_bound(d, nxt, coef, gs)).all())


def _build(cfg, **kw):
    from tacorl_amd import lightning as L

    return L.instantiate(cfg, **kw)


def test_constructors():
    from tests import d4rl_cfg as K

    cql = _build(C.cql_cfg(with_dr3=True, dr3_coefficient=0.3))
    assert cql.engine.dr3 == 0.3 and cql.with_dr3 and cql.hparams["with_dr3"] is True
    off = _build(C.cql_cfg())
    assert off.engine.dr3 is None and not off.with_dr3
    assert sorted(cql.state_dict()) == sorted(off.state_dict())  # the term adds no parameter
    lmp = _build(C.playlmp_cfg())
    tac = _build(C.tacorl_cfg(with_dr3=True), play_lmp=lmp)
    assert tac.engine.dr3 == 0.03
    assert _build(C.tacorl_cfg(), play_lmp=_build(C.playlmp_cfg())).engine.dr3 is None
    for bad in (0.0, -0.03):
        with pytest.raises(ValueError):
            _build(C.cql_cfg(with_dr3=True, dr3_coefficient=bad))
    # the bare switch, coefficient not given, keeps the refusal it had before the term was built (tests/lightning_script.py
    # pins it); given, as the module configs give it - the reference's 0.03 included - it builds
    with pytest.raises(NotImplementedError) as e:
        _build(C.cql_cfg(with_dr3=True))
    assert "dr3_coefficient" in str(e.value)
    assert _build(C.cql_cfg(with_dr3=True, dr3_coefficient=0.03)).engine.dr3 == 0.03
    assert _build(C.cql_cfg()).hparams["dr3_coefficient"] == 0.03  # (the default the hyper-parameters record is unchanged)
    # VIB stays refused, by a message that names VIB alone
    for cfg, kw in ((C.cql_cfg(with_vib=True), {}), (C.tacorl_cfg(with_vib=True), dict(play_lmp=lmp)),
                    (C.cql_cfg(with_vib=True, with_dr3=True), {})):
        with pytest.raises(NotImplementedError) as e:
            _build(cfg, **kw)
        assert "VIB" in str(e.value) and "DR3" not in str(e.value)
    # the D4RL modules: the reference's own critics there cannot compute the term
    dl = K.build(K.playlmp_d4rl_cfg())
    for cfg in (K.cql_d4rl_cfg(with_dr3=True), K.tacorl_d4rl_cfg(play_lmp=dl, with_dr3=True)):
        with pytest.raises(NotImplementedError) as e:
            K.build(cfg)
        assert "get_emb_obs_representation" in str(e.value)
    for cfg in (K.cql_d4rl_cfg(with_vib=True), K.tacorl_d4rl_cfg(play_lmp=dl, with_vib=True)):
        with pytest.raises(NotImplementedError) as e:
            K.build(cfg)
        assert "VIB" in str(e.value)


def test_log_slots_are_appended_and_filtered():
    from tacorl_amd import _lib

    assert _lib.LOG_SLOTS[-2:] == ["q1_dr3_loss", "q2_dr3_loss"] and _lib.LOG_SLOTS.index("action_loss") == 17
    assert tuple(_lib.DR3_SLOTS) == ("q1_dr3_loss", "q2_dr3_loss") and len(_lib.LOG_SLOTS) <= 32
    # the action decoder's loss writes two floats at action_loss: the slot behind it stays unnamed
    assert _lib.LOG_SLOTS[18] is None and _lib.LOG_SLOTS.index("q1_dr3_loss") == 19
