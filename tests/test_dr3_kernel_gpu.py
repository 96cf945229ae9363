"""tacorl_dr3_fwd_bwd alone against tests/dr3_ref.py in fp64, both critics in one launch: every scalar and every gradient
element inside its a-priori bound (derived in dr3_ref's docstring), the gradient ADDED into pre-filled rows, columns >= Eo
bit-untouched, two runs bit-identical, and every refusal returned before any launch.  Row counts on both sides of the 64-lane
wave and of the 256-thread workgroup's stride, both widths, padded and dense rows, both gradient scales."""
import pytest
import torch

from tests import dr3_ref as R
from tests.golden_util import record_margin

pytestmark = pytest.mark.gpu

COEF = 0.03  # the reference default (config/module/tacorl.yaml)
NSLOT = 32
SENT = -7.25  # sentinel of the log record


def _lib():
    from tacorl_amd import _lib as L

    L.call("tacorl_hip_init", 0)
    return L


def _slots(L):
    ix = L.LOG_SLOTS.index
    return [ix("q1_dr3_loss"), ix("q2_dr3_loss")], [ix("q1_loss"), ix("q2_loss")]


def _launch(L, prob, ld, B, Eo, gs, logs, coef=COEF):
    dr3, loss = _slots(L)
    return L.lib().tacorl_dr3_fwd_bwd(2, L.ptr_array([p["obs"] for p in prob]), ld, L.ptr_array([p["next"] for p in prob]), ld,
                                      L.ptr_array([p["d"] for p in prob]), ld, B, Eo, coef, gs, L.ptr(logs), L.int_array(dr3),
                                      L.int_array(loss), L.stream())


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("Eo", [32, 64])
@pytest.mark.parametrize("B", [1, 3, 63, 64, 65, 257])
def test_dr3_kernel_inside_bounds(B, Eo, pad, gs):
    L = _lib()
    dev, ld = torch.device("cuda:0"), Eo + pad
    host = R.problem(B, Eo, ld, 5)
    dr3, loss = _slots(L)
    runs = []
    for _ in range(2):
        prob = [{k: v.to(dev).contiguous() for k, v in p.items()} for p in host]
        logs = torch.full((NSLOT,), SENT, device=dev)
        q_loss = [11.5, -3.25]
        for s, v in zip(loss, q_loss):
            logs[s] = v
        assert _launch(L, prob, ld, B, Eo, gs, logs) == 0
        torch.cuda.synchronize()
        runs.append((logs.cpu(), [p["d"].cpu() for p in prob]))
        for p, h in zip(prob, host):  # the operands are read only
            assert torch.equal(p["obs"].cpu(), h["obs"]) and torch.equal(p["next"].cpu(), h["next"])
    logs, ds = runs[0]
    assert torch.equal(logs, runs[1][0]) and all(torch.equal(a, b) for a, b in zip(ds, runs[1][1])), "two runs differ"
    worst_v = worst_g = 0.0
    for k, h in enumerate(host):
        obs, nxt = h["obs"][:, :Eo], h["next"][:, :Eo]
        v, vb = R.value(obs, nxt, COEF), R.value_bound(obs, nxt, COEF)
        got = float(logs[dr3[k]])
        print(f"B {B} Eo {Eo} ld {ld} gs {gs} critic {k}: value {got:.8g} fp64 {v:.8g} error / bound {abs(got - v) / vb:.3g}")
        worst_v = max(worst_v, abs(got - v) / vb)
        assert abs(got - v) <= vb, (k, got, v, vb)
        # the same fp32 value is added into the critic's loss slot: fl(q_loss + v32), exactly
        assert float(logs[loss[k]]) == float(torch.tensor(q_loss[k], dtype=torch.float32) + logs[dr3[k]])
        ref = h["d"][:, :Eo].double() + R.grad_term(nxt, COEF, gs)
        use = ((ds[k][:, :Eo].double() - ref).abs() / R.grad_bound(h["d"][:, :Eo], nxt, COEF, gs)).max().item()
        print(f"    gradient rows: worst element error / bound {use:.3g}")
        worst_g = max(worst_g, use)
        assert use <= 1.0, (k, use)
        assert torch.equal(ds[k][:, Eo:], h["d"][:, Eo:]), "columns >= Eo of the gradient rows were written"
    others = [i for i in range(NSLOT) if i not in dr3 + loss]
    assert bool((logs[others] == SENT).all()), "a slot of the record that is not the launch's was written"
    record_margin(f"B{B} Eo{Eo} ld{ld} gs{gs}: value", worst_v, 1.0, kind="dr3 kernel (error / bound)")
    record_margin(f"B{B} Eo{Eo} ld{ld} gs{gs}: gradient element", worst_g, 1.0, kind="dr3 kernel (error / bound)")


def test_dr3_kernel_refusals_launch_nothing():
    L = _lib()
    dev, B, Eo, ld = torch.device("cuda:0"), 3, 32, 40
    prob = [{k: v.to(dev).contiguous() for k, v in p.items()} for p in R.problem(B, Eo, ld, 6)]
    d0 = [p["d"].clone() for p in prob]
    logs = torch.full((NSLOT,), SENT, device=dev)
    dr3, loss = _slots(L)
    f = L.lib().tacorl_dr3_fwd_bwd
    obs, nxt, d = (L.ptr_array([p[k] for p in prob]) for k in ("obs", "next", "d"))
    st = L.stream()

    def call(n=2, obs=obs, ld_o=ld, nxt=nxt, ld_n=ld, d=d, ld_d=ld, B=B, Eo=Eo, logs_p=L.ptr(logs), s_dr3=L.int_array(dr3),
             s_loss=L.int_array(loss)):
        return f(n, obs, ld_o, nxt, ld_n, d, ld_d, B, Eo, COEF, 1.0, logs_p, s_dr3, s_loss, st)

    null1 = lambda key: L.ptr_array([prob[0][key], None])  # noqa: E731
    bad = dict(
        n0=call(n=0), n3=call(n=3), B0=call(B=0), Bneg=call(B=-1), Eo0=call(Eo=0), Eo_not_32=call(Eo=24), Eo_48=call(Eo=48, ld_o=64, ld_n=64, ld_d=64),
        ld_obs=call(ld_o=Eo - 1), ld_next=call(ld_n=Eo - 4), ld_d=call(ld_d=Eo - 1), ld_for_64=call(Eo=64),
        obs_null=call(obs=None), next_null=call(nxt=None), d_null=call(d=None), logs_null=call(logs_p=None),
        slots_null=call(s_dr3=None), loss_slots_null=call(s_loss=None), obs1_null=call(obs=null1("obs")),
        next1_null=call(nxt=null1("next")), d1_null=call(d=null1("d")),
        slot_outside=call(s_dr3=L.int_array([dr3[0], 4096])), slot_negative=call(s_dr3=L.int_array([-1, dr3[1]])),
        loss_slot_negative=call(s_loss=L.int_array([loss[0], -1])), loss_slot_outside=call(s_loss=L.int_array([4096, loss[1]])),
        slots_shared=call(s_dr3=L.int_array([dr3[0], dr3[0]])), dr3_is_loss=call(s_dr3=L.int_array(loss)),
        d_shared=call(d=L.ptr_array([prob[0]["d"], prob[0]["d"]])),
    )
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc == 0}
    assert bool((logs == SENT).all()) and all(torch.equal(p["d"], x) for p, x in zip(prob, d0)), "a refused call wrote"
    # ... and the same arguments unspoiled are served
    assert call() == 0
    torch.cuda.synchronize()
    out = logs.cpu()
    assert all(float(out[s]) != SENT for s in dr3 + loss)
    assert not any(torch.equal(p["d"][:, :Eo], x[:, :Eo]) for p, x in zip(prob, d0))
