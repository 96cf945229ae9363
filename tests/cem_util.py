"""Loader of the CEM fixtures (tests/golden/cem_*.npz, made by tools/gen_cem_golden.py from the unmodified reference) and a
plain-torch Q head on their parameters, shared by tests/test_cem_cpu.py and tests/test_cem_gpu.py."""
import numpy as np
import torch

from tacorl_amd import synth
from tests.golden_util import Golden


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rel_gaps(q, n_elite):
    s = np.sort(np.asarray(q, dtype=np.float64))[::-1]
    m = np.abs(s).max()
    return (s[n_elite - 1] - s[n_elite]) / m, (s[0] - s[1]) / m


def order_gap(q, n_elite):
    s = np.sort(np.asarray(q, dtype=np.float64))[::-1]
    return float(np.min(s[: n_elite - 1] - s[1:n_elite]) / np.abs(s).max())


class CemGolden(Golden):
    def __init__(self, name):
        super().__init__(name)
        self.cases = {c["name"]: c for c in self.cfg["cases"]}
        # elite selection is discontinuous: the fixture is only a yardstick while the reference's own Q values keep the
        # selection boundary and the best candidate apart by ten times the fp32 tolerance
        for cname, c in self.cases.items():
            ne = int(np.round(c["batch_size"] * c["elite_fraction"]))
            worst = min(g for q in self.z[f"c/{cname}/q"] for g in rel_gaps(q, ne))
            assert worst >= self.cfg["gap"] and abs(worst - c["min_rel_gap"]) < 1e-9, (name, cname, worst)
            og = min(order_gap(q, ne) for q in self.z[f"c/{cname}/q"])
            assert abs(og - c["min_order_gap"]) < 1e-9, (name, cname, og)

    def params(self):
        P = super().params()
        for k in P:
            if k.startswith(("q1.", "q2.")) and ".critic.Q.out." in k:
                P[k] = P[k] * self.cfg["out_scale"]
        return P

    def obs(self, batched=True):
        """{'observation': {cam: img}, 'goal': {cam: img}} of the one recorded observation, (1,3,H,W) or (3,H,W) images."""
        if self.cfg["kind"] == "cem_tacorl":
            b = synth.make_play_batch(self.cfg["seed"] * 100, 1, 2, self.cams)
            o = {"observation": {k: v[:, 0] for k, v in b["states"].items()}, "goal": b["goal"]}
        else:
            o = synth.make_transition_batch(self.cfg["seed"] * 100, 1, self.cams)["observations"]
        return o if batched else {k: {c: v[0] for c, v in d.items()} for k, d in o.items()}

    def case(self, cname):
        pre = f"c/{cname}/"
        d = {k[len(pre):]: torch.from_numpy(self.z[k]) for k in self.z.files if k.startswith(pre)}
        d["hp"] = self.cases[cname]
        d["n_elite"] = int(np.round(d["hp"]["batch_size"] * d["hp"]["elite_fraction"]))
        d["mean0"] = torch.from_numpy(self.z["actor_mean"]) if d["hp"]["from_actor"] else None
        # the populations are not stored: iteration i's is clamp(mean + std * eps, -1, 1) of the stored state before it
        hp, A = d["hp"], d["hp"]["action_dim"]
        mean = d["mean0"].double() if d["mean0"] is not None else torch.zeros(A, dtype=torch.float64)
        std, pops = torch.full((A,), hp["max_std"], dtype=torch.float64), []
        for it in range(hp["num_iterations"]):
            pop = (mean + d["eps"][it].double() * std).clamp(-1.0, 1.0)
            if hp["discrete_gripper"]:
                pop[:, -1] = torch.where(pop[:, -1] >= 0, 1.0, -1.0).double()
            pops.append(pop)
            mean, std = d["mean"][it].double(), d["std"][it].double()
        d["pop"] = torch.stack(pops).float()
        return d

    def emb(self, which):
        return torch.from_numpy(self.z["emb_" + which])


def same_elite_order(got, want, q, tol):
    """Elite indices `got` against the fixture's `want` (both by descending Q), given the fixture's Q values `q` of that
    iteration: equal position by position, except that a run of neighbouring elites whose Q values are closer than
    tol * max|Q| (closer than the comparison's own tolerance, so they may legitimately swap) is compared as a set."""
    got, want = [int(i) for i in got], [int(i) for i in want]
    if len(got) != len(want):
        return False
    qv = [float(q[i]) for i in want]
    lim = tol * float(torch.as_tensor(q).abs().max())
    i = 0
    while i < len(want):
        j = i + 1
        while j < len(want) and qv[j - 1] - qv[j] < lim:
            j += 1
        if sorted(got[i:j]) != sorted(want[i:j]):
            return False
        i = j
    return True


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def q_head(P, which, dtype=torch.float64, bf16_operands=False):
    """Q(emb (E,), actions (N,A)) -> (N,) of critic `which` ('q1' / 'q2') from the state-dict P: MLPQNetwork, SiLU hidden
    layers (reference critic.py:92-97).  bf16_operands: weights and every layer's input rounded to bf16, biases and
    accumulation in `dtype` - the arithmetic contract of the library's bf16 compute mode."""
    n = 0
    while f"{which}.critic.Q.fc_layers.{n}.weight" in P:
        n += 1
    layers = [(P[f"{which}.critic.Q.fc_layers.{i}.weight"], P[f"{which}.critic.Q.fc_layers.{i}.bias"]) for i in range(n)]
    layers.append((P[f"{which}.critic.Q.out.weight"], P[f"{which}.critic.Q.out.bias"]))
    rnd = _bf if bf16_operands else (lambda t: t)
    layers = [(rnd(w.float()).to(dtype), b.to(dtype)) for w, b in layers]

    def q(emb, actions):
        actions = actions.to(dtype)
        x = torch.cat([emb.to(dtype).reshape(1, -1).expand(actions.shape[0], -1), actions], dim=-1)
        for i, (w, b) in enumerate(layers):
            x = (rnd(x.float()).to(dtype) if bf16_operands else x) @ w.to(x.device).T + b.to(x.device)
            if i + 1 < len(layers):
                x = torch.nn.functional.silu(x)
        return x.reshape(-1)

    return q


def q_fn_of(P, twin, dtype=torch.float64, bf16_operands=False):
    """q_fn for cem_restatement with emb = (emb_q1, emb_q2): q1, or min(q1, q2)."""
    q1, q2 = q_head(P, "q1", dtype, bf16_operands), q_head(P, "q2", dtype, bf16_operands)
    if not twin:
        return lambda emb, a: q1(emb[0], a)
    return lambda emb, a: torch.minimum(q1(emb[0], a), q2(emb[1], a))
