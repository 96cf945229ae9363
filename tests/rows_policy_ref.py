"""fp64 restatement of tacorl_rows_mlp_fwd (tacorl_amd/csrc/rollout_ops.hip) - an MLP chain for a handful of rows whose last
layer is an ordinary one (mode "plain") or a policy head read as the deterministic action (mode "policy action") - and the
a-priori bounds the kernel is held to.  Plain torch on the CPU: no GPU, no kernel of this repository.

Per layer, on that layer's OWN input h (what the kernel itself fed it, so that an error does not cascade):

    |y - y64| <= lip(act) * gamma_{K+4} * (|b| + sum |w||h|) + act_tolerance(act, z64)

gamma and the linear bound are tests/rows_linear_ref.py's (the hidden layers ARE that kernel), act_tolerance is
tests/mlp_ref.py's, lip = 1 but for SiLU, whose slope reaches 1.0998: the 1.1 of tests/mlp_ref.py's stage_checks.  The action
columns are tanh (1-Lipschitz) of the mean rows of the head; the gripper column is +1 where logit 1 > logit 0, else -1, and is
compared EXACTLY: the seeded problems draw the gripper head at randn / sqrt(K) scale, and tests/test_rows_policy_ref_cpu.py
shows that every row used has an fp64 logit gap above GAP_RATIO x the two logits' summed bounds, so no row is skipped.
Nothing here is tuned to a kernel's output."""
import torch

from tests import rows_linear_ref as RL
from tests.mlp_ref import ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH, act, act_tolerance
from tests.rows_linear_ref import gamma

SILU_LIP = 1.1      # tests/mlp_ref.py stage_checks: the sum's bound times the activation's Lipschitz constant (1; SiLU 1.1)
FAULT_RATIO = 10.0  # every fault of tests/test_rows_policy_ref_cpu.py exceeds its bound by this factor
GAP_RATIO = 10.0    # every row's fp64 logit gap exceeds this many times the two logits' summed bounds
PAD = 7.0           # what the padding columns of x and y hold
MEAN_CLAMP = 9.0    # reference actor.py:14-15

# chains E -> H x L -> head, and the heads (Ac, discrete gripper)
SHAPES = [(45, 70, 2), (64, 72, 1)]
REAL_SHAPE = (64, 1024, 4)  # the configured 4 x 1024 (config/module/relay_imitation_learning.yaml) behind [32 | 32]: run once
HEADS = [(6, True), (32, False)]
ROWS = [1, 2, 3, 5, 8, 9, 16, 17, 64]  # the NR = 1 / 2 / 4 / 8 switches and the group edges
REAL_ROWS = 9
MAX_ROWS = 64
SUB_COLS = 16  # the trailing input columns that stand for the sub-goal (the 'subgoal_row' fault)


def lip(a):
    return SILU_LIP if a == ACT_SILU else 1.0


def linear_bound(K, scale):
    """rows_linear_ref.bound for a layer without x2: gamma_{K+4} * scale."""
    return RL.bound(dict(K1=K, K2=0, x2=None), scale)


_cache = {}


def problem(shape, head, seed=0, pad=3):
    """The seeded MAX_ROWS-row problem of a chain (the R-row cases are its first R rows): x (64, E + pad) fp32 with the pad
    columns = PAD, SiLU hidden layers W [l] = randn / sqrt(K), b = 0.1 randn, the head [mean (Ac) | log-std (Ac) | gripper (2)]
    at the same randn / sqrt(K) scale.  Computed once per (shape, head, seed) and never modified."""
    key = (shape, head, seed)
    if key not in _cache:
        (E, H, L), (Ac, dg) = shape, head
        g = torch.Generator().manual_seed(100003 * seed + 1009 * E + 31 * H + 7 * L + 3 * Ac + int(dg))
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
        dims = [E] + [H] * L + [2 * Ac + (2 if dg else 0)]
        x = torch.full((MAX_ROWS, E + pad), PAD)
        x[:, :E] = rn(MAX_ROWS, E)
        W = [rn(dims[l + 1], dims[l]) / dims[l] ** 0.5 for l in range(L + 1)]
        b = [rn(dims[l + 1]) * 0.1 for l in range(L + 1)]
        _cache[key] = dict(E=E, H=H, L=L, Ac=Ac, dg=dg, A=Ac + int(dg), dims=dims, acts=[ACT_SILU] * L + [ACT_NONE], x=x, W=W, b=b)
    return _cache[key]


def fault_neuron(p, l):
    """The neuron of the 'bias' fault: the one of layer l with the largest |b| (a seeded bias can be arbitrarily near zero)."""
    return int(p["b"][l].abs().argmax())


def linear64(p, l, h, rows=None):
    """(z, scale) in fp64 of layer l on input h (n, K): z = h W^T + b and |b| + sum |w||h|; rows: the weight rows to take."""
    W, b = p["W"][l].double(), p["b"][l].double()
    if rows is not None:
        W, b = W[rows], b[rows]
    h = h.double()
    return h @ W.t() + b, h.abs() @ W.abs().t() + b.abs()


def layer_ref(p, l, h, a=None):
    """(y64, bound) of layer l with activation a (default: the chain's) on its own input h."""
    a = p["acts"][l] if a is None else a
    z, s = linear64(p, l, h)
    return act(a, z), lip(a) * linear_bound(h.shape[1], s) + act_tolerance(a, z)[0]


def mean_rows(p):
    return list(range(p["Ac"]))


def logit_rows(p):
    return [2 * p["Ac"], 2 * p["Ac"] + 1]


def action_ref(p, h):
    """The policy-action epilogue on the head's own input h (n, H): (action (n, A) fp64 with the gripper column +-1, bound of
    the Ac tanh columns, logits (n, 2) or None, the two logits' bounds)."""
    z, s = linear64(p, p["L"], h, mean_rows(p))
    zc = z.clamp(-MEAN_CLAMP, MEAN_CLAMP)
    out, bnd = torch.tanh(zc), linear_bound(h.shape[1], s) + act_tolerance(ACT_TANH, zc)[0]
    if not p["dg"]:
        return out, bnd, None, None
    lg, ls = linear64(p, p["L"], h, logit_rows(p))
    grip = torch.where(lg[:, 1] > lg[:, 0], 1.0, -1.0).to(out.dtype)  # a tie goes to -1: torch.argmax picks index 0
    return torch.cat([out, grip.unsqueeze(1)], dim=1), bnd, lg, linear_bound(h.shape[1], ls)


def restate(p, R, fault=None, dtype=torch.float64):
    """The whole chain on rows [0, R) of p, every layer on the previous layer's output in `dtype`.  Returns
    dict(h [l]: layer l's input, y [l]: the hidden layers' outputs, action (R, A), logits).  fault: None, or one of
      'logstd'       mean neuron 0 computed from log-std row 0 of the head
      'grip_sign'    the gripper column's sign flipped
      'subgoal_row'  row 0 served row 1's last SUB_COLS input columns (needs R >= 2)
      'tail'         the last input column of layer 0 dropped
      'bias'         the last hidden layer's bias omitted for neuron fault_neuron(p, L - 1)"""
    E, L, Ac = p["E"], p["L"], p["Ac"]
    h = p["x"][:R, :E].to(dtype).clone()
    if fault == "subgoal_row":
        h[0, E - SUB_COLS:] = h[1, E - SUB_COLS:]
    out = dict(h=[], y=[])
    for l in range(L):
        out["h"].append(h)
        W, b = p["W"][l].to(dtype), p["b"][l].to(dtype).clone()
        if fault == "bias" and l == L - 1:
            b[fault_neuron(p, l)] = 0.0
        z = h @ W.t() + b
        if fault == "tail" and l == 0:
            z = z - h[:, -1:] * W[:, -1]
        h = act(p["acts"][l], z)
        out["y"].append(h)
    out["h"].append(h)
    W, b = p["W"][L].to(dtype), p["b"][L].to(dtype)
    rows = mean_rows(p)
    if fault == "logstd":
        rows = [Ac] + rows[1:]
    a = torch.tanh((h @ W[rows].t() + b[rows]).clamp(-MEAN_CLAMP, MEAN_CLAMP))
    out["logits"] = None
    if p["dg"]:
        lg = h @ W[logit_rows(p)].t() + b[logit_rows(p)]
        grip = torch.where(lg[:, 1] > lg[:, 0], 1.0, -1.0).to(dtype)
        a = torch.cat([a, (-grip if fault == "grip_sign" else grip).unsqueeze(1)], dim=1)
        out["logits"] = lg
    out["action"] = a
    return out


def gap_margin(p, R):
    """Per row of rows [0, R): the fp64 logit gap |l1 - l0| over the two logits' summed bounds, on the fp64 chain's own last
    hidden layer.  Above GAP_RATIO for every row, the gripper column can be compared exactly."""
    h = restate(p, R)["h"][-1]
    _, _, lg, lb = action_ref(p, h)
    return (lg[:, 1] - lg[:, 0]).abs() / lb.sum(dim=1)


def cases():
    """(shape, head, R) of tests/test_rows_policy_gpu.py."""
    out = [(s, hd, R) for s in SHAPES for hd in HEADS for R in ROWS]
    return out + [(REAL_SHAPE, HEADS[0], REAL_ROWS)]
