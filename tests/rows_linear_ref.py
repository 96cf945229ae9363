"""fp64 restatement of tacorl_rows_linear2_fwd (tacorl_amd/csrc/rollout_ops.hip) and the a-priori bound the kernel is held to,
in the manner of tests/mlp_ref.py.  Plain torch on the CPU: no GPU, no kernel of this repository.

    y[r][n] = act(b1[n] + b2[n] + sum_k w1[n][k] x1[r][k] + sum_k w2[n][k] x2[r][k])

with row r of x2 taken as zeros where flags[r] != 0.  The kernel adds the K1 + K2 products in fp32 FMAs (one rounding each),
sums 64 lane partials by a butterfly and adds the two biases: every order of those K1 + K2 + 2 additions is covered by
the classical bound of a recursive fp32 sum,

    |y - y64| <= gamma_{K1+K2+4} (|b1| + |b2| + sum |w||x|),   gamma_n = n u / (1 - n u),   u = 2^-24,

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1/4.2; the 4 leaves room for the roundings of the inputs'
fp64 -> fp32 representation - none here, the operands ARE fp32 - and of the biases).  ReLU is 1-Lipschitz and exact, so the
bound passes through it.  It is derived, not tuned."""
import torch

ACT_NONE, ACT_RELU = 0, 1
U32 = 2.0 ** -24
FAULT_RATIO = 10.0  # every fault of tests/test_rows_linear_ref_cpu.py exceeds the bound by this factor

SHAPES_K = [(45, 72), (48, 0), (72, 72), (257, 259)]
SHAPES_N = [1, 7, 182, 240]
PAD = 7.0  # what the padding columns of x1, x2 and y hold


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def problem(R, K1, K2, N, seed, with_b2=True, flag_rows=(), pad=3):
    """A seeded problem in fp32 (the kernel's operands): x1 (R, K1 + pad), x2 (R, K2 + pad) with the pad columns = PAD, weights at
    torch's nn.RNN scale, flags (R,) uint8."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    p = dict(R=R, K1=K1, K2=K2, N=N)
    p["x1"] = torch.full((R, K1 + pad), PAD)
    p["x1"][:, :K1] = rn(R, K1)
    p["w1"], p["b1"] = rn(N, K1) / max(K1, 1) ** 0.5, rn(N) * 0.1
    if K2 > 0:
        p["x2"] = torch.full((R, K2 + pad), PAD)
        p["x2"][:, :K2] = rn(R, K2).abs()  # a hidden state: post-ReLU
        p["w2"] = rn(N, K2) / K2 ** 0.5
    else:
        p["x2"] = p["w2"] = None
    p["b2"] = rn(N) * 0.1 if with_b2 else None
    flags = torch.zeros(R, dtype=torch.uint8)
    for r in flag_rows:
        flags[r] = 1
    p["flags"] = flags if len(flag_rows) else None
    return p


def fault_neuron(p):
    """The neuron of the 'b2' fault: the one with the largest |b2| (a seeded bias can be arbitrarily close to zero)."""
    return int(p["b2"].abs().argmax())


def restate(p, act, dtype=torch.float64, fault=None):
    """(y, scale) in `dtype`: the layer and sum |w||x| + |b1| + |b2|, the bound's scale.  fault: None, or one of
    'tail' (the last element of the x1 product of row 0 dropped), 'row' (row 0 served row 1's x2), 'b2' (neuron
    fault_neuron(p) without b2)."""
    K1, K2 = p["K1"], p["K2"]
    d = lambda t: t.to(dtype)  # noqa: E731
    x1, w1 = d(p["x1"][:, :K1]), d(p["w1"])
    z, s = x1 @ w1.T, x1.abs() @ w1.abs().T
    if fault == "tail":
        z[0] -= x1[0, K1 - 1] * w1[:, K1 - 1]
    z, s = z + d(p["b1"]), s + d(p["b1"]).abs()
    if p["x2"] is not None and K2 > 0:
        x2 = d(p["x2"][:, :K2]).clone()
        if p["flags"] is not None:
            x2[p["flags"].bool()] = 0.0
        if fault == "row":
            x2[0] = x2[1]
        w2 = d(p["w2"])
        z, s = z + x2 @ w2.T, s + x2.abs() @ w2.abs().T
    if p["b2"] is not None:
        b2 = d(p["b2"]).clone().expand(z.shape[0], -1).clone()
        s = s + b2.abs()
        if fault == "b2":
            b2[:, fault_neuron(p)] = 0.0
        z = z + b2
    return (torch.relu(z) if act == ACT_RELU else z), s


def bound(p, scale):
    """The a-priori bound per element (fp64)."""
    return gamma(p["K1"] + (p["K2"] if p["x2"] is not None else 0) + 4) * scale
