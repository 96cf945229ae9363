"""CEM plan refinement without a GPU: the plain-torch restatement against traces recorded from the unmodified reference
CEMOptimizer (tests/golden/cem_*.npz), the fixtures' gap condition, constructor / argument checks, and the C entry points'
argument validation (nothing is launched)."""
import ctypes as C
import types

import pytest
import torch

from tests.cem_util import CemGolden, q_fn_of, rel

CASES = {"cem_cql": ("n64_actor", "n64_actor_twin", "n64_zero", "n64_zero_twin", "n256_actor", "n256_zero_twin"),
         "cem_tacorl": ("n64_actor_twin", "n64_zero", "n256_actor", "n256_zero_twin")}
FILES = tuple(CASES)
FILE_CASES = [(f, c) for f in FILES for c in CASES[f]]


@pytest.mark.parametrize("name", FILES)
def test_fixture_gap_condition_and_coverage(name):
    """Loading asserts the stored gaps (>= 1e-3 max|Q| at the elite boundary and at the top, every iteration of every case,
    and the recorded smallest gap between neighbouring elites); each file covers both population sizes, both starting means and
    both Q forms, and every (starting mean, Q form) pair."""
    g = CemGolden(name)
    assert g.cfg["gap"] == 1e-3 and g.cfg["order_gap"] == 1e-4 and set(g.cases) == set(CASES[name])
    assert {(c["from_actor"], c["twin_min"]) for c in g.cases.values()} == {(a, b) for a in (True, False) for b in (True, False)}
    hp = list(g.cases.values())
    assert {c["batch_size"] for c in hp} == {64, 256} and {c["from_actor"] for c in hp} == {True, False}
    assert {c["twin_min"] for c in hp} == {True, False}
    assert all(c["discrete_gripper"] == (name == "cem_cql") and c["action_dim"] == (7 if name == "cem_cql" else 16) for c in hp)
    assert all(c["min_rel_gap"] >= 1e-3 and c["min_order_gap"] > 0 for c in hp)


@pytest.mark.parametrize("name,cname", FILE_CASES)
def test_restatement_reproduces_reference_trace(name, cname):
    """cem_restatement in fp64 on the recorded draws: the reference's elite indices exactly (in order), its Q, mean, std
    and returned action within 1e-6 (the population is derived from the stored mean, std and draws, see cem_util)."""
    from tacorl_amd.modules.cem import cem_restatement

    g = CemGolden(name)
    c = g.case(cname)
    hp = c["hp"]
    q_fn = q_fn_of(g.params(), hp["twin_min"], torch.float64)
    mean0 = c["mean0"].double() if c["mean0"] is not None else None
    act, tr = cem_restatement(q_fn, (g.emb("q1"), g.emb("q2")), mean0, c["eps"].double(), n_elite=c["n_elite"],
                              min_std=hp["min_std"], max_std=hp["max_std"], alpha=hp["alpha"],
                              discrete_gripper=hp["discrete_gripper"])
    for it in range(hp["num_iterations"]):
        assert torch.equal(tr["elite"][it].int(), c["elite"][it]), (it, tr["elite"][it], c["elite"][it])
        for k in ("q", "mean", "std"):
            e = rel(tr[k][it], c[k][it])
            print(f"{name}/{cname} iteration {it} {k}: rel {e:.3g}")
            assert e < 1e-6, (it, k, e)
    e = rel(act, c["action"])
    print(f"{name}/{cname} action: rel {e:.3g}")
    assert e < 1e-6
    if hp["discrete_gripper"]:
        assert float(act[-1]) == float(c["action"][-1]) and abs(float(act[-1])) == 1.0


def test_restatement_host_sync_form_is_the_same_algorithm():
    from tacorl_amd.modules.cem import cem_restatement

    g = CemGolden("cem_cql")
    c = g.case("n64_zero")
    q_fn = q_fn_of(g.params(), False, torch.float64)
    kw = dict(n_elite=c["n_elite"], discrete_gripper=True)
    a0, _ = cem_restatement(q_fn, (g.emb("q1"), g.emb("q2")), None, c["eps"].double(), **kw)
    a1, _ = cem_restatement(q_fn, (g.emb("q1"), g.emb("q2")), None, c["eps"].double(), host_sync=True, **kw)
    assert torch.equal(a0, a1)


def _fake_critics(A=7, E=64, hidden=256, q_layers=3):
    """Critic surfaces over a stand-in owner: what the constructor checks needs no device."""
    from tacorl_amd._lib import F32
    from tacorl_amd.modules.inference import CriticSurface

    owner = types.SimpleNamespace(dev=torch.device("cpu"), compute=F32, img_dtype=torch.float32)
    net = types.SimpleNamespace(head_dims=[E + A] + [hidden] * q_layers + [1])
    return CriticSurface(owner, net, ["rgb_static"], ["rgb_static"], A), CriticSurface(owner, net, ["rgb_static"], ["rgb_static"], A)


def test_constructor_checks():
    from tacorl_amd.modules.cem import CEMOptimizer

    q1, q2 = _fake_critics()
    cem = CEMOptimizer(q1, q2)
    assert (cem.batch_size, cem.num_iterations, cem.n_elite, cem.twin_min) == (256, 4, 26, False)
    assert CEMOptimizer(q1, q2, batch_size=64).n_elite == 6
    with pytest.raises(TypeError, match="q1"):
        CEMOptimizer(torch.nn.Linear(71, 1), q2)
    with pytest.raises(TypeError, match="q2"):
        CEMOptimizer(q1, lambda o, a: a)
    with pytest.raises(ValueError, match="elite"):
        CEMOptimizer(q1, q2, batch_size=64, elite_fraction=0.02)  # 1 elite: the reference's std would be NaN
    with pytest.raises(ValueError):
        CEMOptimizer(q1, q2, action_dim=8)
    for kw in (dict(batch_size=100), dict(batch_size=512), dict(batch_size=32, elite_fraction=0.5)):
        with pytest.raises(NotImplementedError, match="batch_size"):
            CEMOptimizer(q1, q2, **kw)
    with pytest.raises(NotImplementedError, match="action_dim"):
        CEMOptimizer(*_fake_critics(A=40), action_dim=40)
    with pytest.raises(NotImplementedError, match="hidden"):
        CEMOptimizer(*_fake_critics(hidden=128))
    with pytest.raises(NotImplementedError):
        CEMOptimizer(*_fake_critics(q_layers=1))
    # the three in-scope shapes: CQL, TACORL, C4
    for A, E in ((7, 64), (16, 64), (32, 128)):
        for N in (64, 256):
            CEMOptimizer(*_fake_critics(A=A, E=E), batch_size=N, action_dim=A)


def test_entry_points_answer_and_refuse_without_gpu():
    """tacorl_cem_supported / _ws_bytes answer for the in-scope shapes in both compute modes; tacorl_cem_refine validates
    its arguments before it touches the device (every call below is refused, so nothing is launched here)."""
    from tacorl_amd import _lib

    L = _lib.lib()
    for A, E in ((7, 64), (16, 64), (32, 128)):
        for N in (64, 256):
            for compute in (_lib.F32, _lib.BF16):
                assert L.tacorl_cem_supported(N, A, E, 256, 3, compute) == 1
                assert L.tacorl_cem_ws_bytes(16, N, A, E, 256, 3, compute) == 4 * 16 * (1 + 2 * A)
    assert L.tacorl_cem_supported(100, 7, 64, 256, 3, 0) == 0 and L.tacorl_cem_supported(512, 7, 64, 256, 3, 0) == 0
    assert L.tacorl_cem_supported(256, 33, 64, 256, 3, 0) == 0 and L.tacorl_cem_supported(256, 7, 64, 128, 3, 0) == 0
    assert L.tacorl_cem_supported(256, 7, 64, 256, 1, 0) == 0 and L.tacorl_cem_supported(256, 7, 64, 256, 3, 2) == 0
    assert L.tacorl_cem_ws_bytes(1, 100, 7, 64, 256, 3, 0) == 0 and L.tacorl_cem_ws_bytes(0, 256, 7, 64, 256, 3, 0) == 0

    P2 = C.c_void_p * 2
    ok, p = P2(4096, 8192), C.c_void_p(4096)  # (never dereferenced)

    def refine(R=1, nnet=1, s=ok, params=ok, mirror=None, eps=p, out=p, N=256, A=7, E=64, hidden=256, layers=3, iters=4,
               n_elite=26, min_std=1e-3, max_std=0.3, alpha=0.1, compute=0, ws=p, ws_bytes=1 << 20):
        return L.tacorl_cem_refine(R, nnet, s, params, mirror, None, eps, out, N, A, E, hidden, layers, iters, n_elite, min_std,
                                   max_std, alpha, 0, compute, None, None, None, None, None, ws, ws_bytes, None)

    bad = [dict(R=0), dict(nnet=0), dict(nnet=3), dict(N=100), dict(A=33), dict(E=0), dict(hidden=512), dict(layers=5),
           dict(iters=0), dict(n_elite=1), dict(n_elite=257), dict(min_std=0.0), dict(max_std=1e-4), dict(alpha=1.5),
           dict(eps=None), dict(out=None), dict(ws=None), dict(ws_bytes=8), dict(s=None), dict(params=None),
           dict(params=P2(4100, 8192)), dict(compute=1), dict(compute=1, mirror=P2(4098, 8192)), dict(nnet=2, s=P2(4096, 0))]
    for kw in bad:
        assert refine(**kw) != 0, kw


def test_header_ctypes_table_and_library_agree():
    """Argument by argument: the C types of the header's CEM prototypes are the ctypes entries of the binding."""
    import os
    import re

    from tacorl_amd import _lib

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl or "tacorl_stream_t" in decl:
            return C.c_void_p
        for word, ct in (("size_t", C.c_size_t), ("float", C.c_float), ("long", C.c_long), ("int", C.c_int)):
            if re.search(r"\b" + word + r"\b", decl):
                return ct
        raise AssertionError(decl)

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "tacorl_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("tacorl_cem_supported", "tacorl_cem_ws_bytes", "tacorl_cem_refine"):
        m = re.search(r"([A-Za-z_][A-Za-z_0-9 ]*?)\b" + name + r"\s*\(([^;]*)\)\s*;", txt, flags=re.S)
        assert m, name
        res, args = _lib._SIGS[name]
        assert ctype_of(m.group(1)) is res, (name, m.group(1))
        got = [ctype_of(a) for a in m.group(2).split(",")]
        assert got == list(args), (name, [(i, a.strip()) for i, (a, x, y) in enumerate(zip(m.group(2).split(","), got, args)) if x is not y])
        assert hasattr(L, name)
    # the float arguments sit where the header puts them
    assert [i for i, a in enumerate(_lib._SIGS["tacorl_cem_refine"][1]) if a is C.c_float] == [15, 16, 17]


def test_same_elite_order_helper():
    """The order comparison of the GPU trace test: exact where neighbours are apart, a set inside a near-tie run only."""
    from tests.cem_util import same_elite_order

    q = torch.tensor([1.0, 0.5, 0.49999, 0.2, -1.0, 0.1])
    want = [0, 1, 2, 3]
    assert same_elite_order([0, 1, 2, 3], want, q, 1e-4) and same_elite_order([0, 2, 1, 3], want, q, 1e-4)
    assert not same_elite_order([1, 0, 2, 3], want, q, 1e-4) and not same_elite_order([0, 1, 3, 2], want, q, 1e-4)
    assert not same_elite_order([0, 2, 1, 3], want, q, 1e-6) and not same_elite_order([0, 1, 2, 5], want, q, 1e-4)
