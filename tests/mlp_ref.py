"""fp64 restatement of the fused MLP chain (Linear + {NONE, ReLU, SiLU, TANH} layers: tacorl_amd/csrc/mlp_fused.hip and the
per-layer path of dense_ops.hip), stage by stage, with the rounding points of the HIP kernels, seeded problems that make
its checks discriminating, the a-priori bounds of an fp32 accumulation and the constants tests/test_mlp_fp64_gpu.py holds
the kernels to (tests/test_mlp_ref_cpu.py shows what those constants still detect).  Plain torch on the CPU: no GPU, no
kernel of this repository; the oracle is one of the things compared against this file.

Rounding points, read from the kernels (bf16 mode; every rounding is round-to-nearest-even, `(__bf16)x`):
  x                 bf16 when staged into the LDS (mlp_fused.hip:146 / :169 / :172; many rows :818, persistent :1069)
  W                 bf16 MFMA operand: the bf16 mirror of the parameter block (load_w, mlp_fused.hip:81); the transposed
                    copy of the backward is rounded by pack_wt_tiles (:306)
  b                 fp32, added to the finished sum (:234, :879, :903)
  hidden y          fp32 act(z) (act_fast, :61), saved as such by the few-row kernels; re-rounded to bf16 as the next
                    layer's operand (:248).  Many-row lean problems save exactly that bf16 value (:887 -> :937) and
                    act'(z) as fp16 (:888 -> :938), zero rows up to the padded row count
  d_out             bf16 when staged (:383, many rows :1259, persistent DQ :1437, last-layer weight gradient :1773).  A TANH
                    output layer first forms dZ = d_out (1 - y^2) in fp32 (dense_ops.hip out_act_grad_kernel)
  dZ_l              fp32 acc * act'(z) (fp32 act' :443, fp16 act' :1323 / :1460 / :1518), stored fp32 by the few-row chain
                    (:455) and bf16 by the many-row one (:1346, :1462); rounded to bf16 before the next product either
                    way (:462, :1337)
  d_x               the fp32 accumulator, not rounded (:455, :1330)
  dW_l, db_l        bf16(dZ_l)^T bf16(input_l); the bias gradient rides on the same MFMA against ones, i.e. it is the sum
                    of the ROUNDED dZ_l on every bf16 path (:606, :1688, :1780); fp32 sums, reduced in slice order (:650)
f32 mode (`rounded=False`): no rounding anywhere (the per-layer path with fp32 MFMA)."""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH = 0, 1, 2, 3

U32 = 2.0 ** -24    # unit roundoff of fp32
C_SUM = 2.0         # stage / additivity: |got - ref| <= C_SUM * K * U32 * (sum |x||w| + |b|), as tests/encoder_ref.py
ACT_FACTOR = 4.0    # act(z), act'(z): 4 x the error of plain fp32 torch on the same z (floor: 1 fp32 ulp of the value)
E2E_FACTOR = 4.0    # F2: 4 x the fp32 rounded oracle's worst row
GRAD_FACTOR = 4.0   # B1 / B2: 4 x the fp32 rounded oracle's error on the slice class
FAULT_RATIO = 10.0  # every fault of tests/test_mlp_ref_cpu.py exceeds its bound by this factor
PAD = 7.0           # what the pad columns of x hold

# the project's MLP sites: (dims, acts, row pitch of x)
SITES = {
    "q_head": ([71, 256, 256, 256, 1], [2, 2, 2, 0], 72),
    "actor_head": ([80, 256, 256, 256, 14], [2, 2, 2, 0], 80),
    "goal_enc": ([32, 256, 256, 32], [1, 1, 0], 32),
    "goal_enc_tanh": ([32, 256, 256, 32], [1, 1, 3], 32),
    "q3": ([80, 256, 256, 3], [2, 2, 0], 80),
    "narrow": ([64, 128, 24], [2, 0], 64),
}
BIG_ROWS, HUGE_ROWS = 2048, 16384  # mlp_fused.hip MLP_BIG_ROWS, mlp_rows_huge
SAT_ROW, SAT_SCALE = 5, 64.0       # the deliberately saturated row of a TANH problem (present when M > SAT_ROW)


def many_row_site(site):
    """mlp_big_prob_ok: the lean many-row kernels take this site at >= 2048 rows."""
    dims, acts, _ = SITES[site]
    return (len(dims) >= 3 and 8 <= dims[0] <= 128 and dims[-1] <= 4 and all(d == 256 for d in dims[1:-1])
            and all(a == ACT_SILU for a in acts[:-1]) and acts[-1] == ACT_NONE)


def regime(site, M, lean=True):
    """'small' (< 2048 rows, or a site the many-row kernels do not take), 'mid' (32-row workgroups, bf16 / fp16 saves) or
    'huge' (>= 16384 rows: 128 / 64-row or persistent workgroups, the same saves)."""
    if not (lean and many_row_site(site)) or M < BIG_ROWS:
        return "small"
    return "huge" if M >= HUGE_ROWS else "mid"


def padded(M):
    return (M + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------- rounding
def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def fp16(t):
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


def _ulp(t, bits):
    t = t.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(t)) - bits)


def bf16_ulp(t):
    return _ulp(t, 7)


def fp16_ulp(t):
    return _ulp(t, 10).clamp_min(2.0 ** -24)


def _r(t, rounded):
    return bf16(t) if rounded else t


# --------------------------------------------------------------------------------------------- activations
def act(a, z):
    return [z, F.relu(z), F.silu(z), torch.tanh(z)][a]


def act_grad(a, z, y):
    """act'(z); ReLU and TANH from the saved output, as the kernels take it."""
    if a == ACT_RELU:
        return (y > 0).to(z.dtype)
    if a == ACT_SILU:
        sg = torch.sigmoid(z)
        return sg * (1 + z * (1 - sg))
    if a == ACT_TANH:
        return 1 - y * y
    return torch.ones_like(z)


def act_tolerance(a, z, fn=None):
    """Per-element tolerance of a fast-exp activation evaluated on the fp32 z: ACT_FACTOR x the worst error of plain fp32
    torch on the same z, at least one fp32 ulp of the value.  -> (tolerance, torch's worst error)."""
    fn = fn or (lambda t: act(a, t))
    ref = fn(z.double())
    e32 = float((fn(z.float()).double() - ref).abs().max()) if z.numel() else 0.0
    return torch.maximum(torch.full_like(ref, ACT_FACTOR * e32), 2 * U32 * ref.abs()), e32


# ------------------------------------------------------------------------------------------------ problems
def problem(site, M, seed=0):
    """{dims, acts, ld, W [l], b [l], x (M, ld) fp32 with the pad columns at PAD, d_out (M, NL)}: seeded, uniform weights of
    variance 1 / K (half that scale in front of a TANH: outputs spread without saturating), biases +-0.1, x in [-1, 1],
    d_out in [-0.5, 1.5] (mean 0.5: a zero-mean d_out makes the bias sums cancellations, test_kernels_gpu.py:722).
    A TANH problem with more than SAT_ROW rows has row SAT_ROW of x scaled by SAT_SCALE: saturated outputs."""
    dims, acts, ld = SITES[site]
    g = torch.Generator().manual_seed(1000 * (sorted(SITES).index(site) + 1) + seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    W = [u(dims[l + 1], dims[l]) * (0.5 if acts[l] == ACT_TANH else 1.0) * math.sqrt(3.0 / dims[l]) for l in range(len(acts))]
    for l in range(1, len(acts)):  # behind a ReLU every input is >= 0: zero-mean weight rows keep each neuron on both sides of 0
        if acts[l - 1] == ACT_RELU:
            W[l] = (W[l] - W[l].mean(1, keepdim=True)) * 1.5
    b = [u(dims[l + 1]) * 0.1 for l in range(len(acts))]
    x = torch.full((M, ld), PAD)
    x[:, :dims[0]] = rows(site, M, seed)
    d_out = torch.rand(M, dims[-1], generator=g) * 2 - 0.5
    return dict(site=site, M=M, dims=dims, acts=acts, ld=ld, W=W, b=b, x=x, d_out=d_out)


def rows(site, M, seed=0):
    """The (M, K0) input rows of problem(site, M, seed): row r depends on (site, seed, r) only in blocks of 4096, so a
    problem's first rows do not change with M."""
    dims, acts, _ = SITES[site]
    out = torch.empty(M, dims[0])
    for blk in range((M + 4095) // 4096):
        g = torch.Generator().manual_seed(77777 * (sorted(SITES).index(site) + 1) + 131 * seed + blk)
        out[blk * 4096: (blk + 1) * 4096] = (torch.rand(4096, dims[0], generator=g) * 2 - 1)[: M - blk * 4096]
    if acts[-1] == ACT_TANH and M > SAT_ROW:
        out[SAT_ROW] *= SAT_SCALE
    return out


def accumulate_base(numel, seed):
    return torch.rand(numel, generator=torch.Generator().manual_seed(seed)) - 0.5


# ----------------------------------------------------------------------------------------- forward / backward
def forward(params, x, dims, acts, rounded=True, dtype=torch.float64, saves="fp32", hook=None):
    """Every stage in `dtype`.  params = (W [l], b [l]); x (M, K0) without pad columns.  -> {h [l]: layer l's operand as
    the MFMA reads it, z [l], y [l], out} and, saves='lean' (the many-row format), {ybf [l], s16 [l]} of the hidden layers:
    bf16 y and fp16 act'(z).  hook(name, l, tensor) -> tensor may replace a stage's result (fault injection)."""
    W, b = params
    hook = hook or (lambda name, l, t: t)
    L = len(acts)
    r = dict(h=[], z=[], y=[], ybf=[], s16=[])
    h = hook("h", 0, _r(x.to(dtype), rounded))
    for l in range(L):
        r["h"].append(h)
        z = hook("z", l, h @ _r(W[l].to(dtype), rounded).t() + b[l].to(dtype))
        y = hook("y", l, act(acts[l], z))
        r["z"].append(z)
        r["y"].append(y)
        if l + 1 < L:
            h = _r(y, rounded)
            if saves == "lean":
                r["ybf"].append(h)
                r["s16"].append(hook("s16", l, fp16(act_grad(acts[l], z, y))))
    r["out"] = r["y"][-1]
    return r


def backward(params, x, d_out, dims, acts, rounded=True, dtype=torch.float64, saves="fp32", fwd=None, want_terms=False, hook=None):
    """{dx, dW [l], db [l], dz [l]} of sum(out * d_out) with the kernels' operand rounding (module docstring), in `dtype`.
    fwd: a forward() result to differentiate at (default: this module's).  want_terms: also terms = {dW [l], db [l]}: the
    sum of the magnitudes of the terms of every gradient element, the scale of the fp32 sum that produces it."""
    W, b = params
    L = len(acts)
    hook = hook or (lambda name, l, t: t)
    f = fwd or forward(params, x, dims, acts, rounded, dtype, saves)
    dz = d_out.to(dtype)
    if acts[-1] != ACT_NONE:
        dz = dz * hook("s", L - 1, act_grad(acts[-1], f["z"][-1], f["y"][-1]))
    out = dict(dW=[None] * L, db=[None] * L, dz=[None] * L)
    terms = dict(dW=[None] * L, db=[None] * L)
    for l in range(L - 1, -1, -1):
        out["dz"][l] = dz
        g = hook("g", l, _r(dz, rounded))
        out["dW"][l], out["db"][l] = g.t() @ f["h"][l], g.sum(0)
        if want_terms:
            terms["dW"][l], terms["db"][l] = g.abs().t() @ f["h"][l].abs(), g.abs().sum(0)
        dA = g @ _r(W[l].to(dtype), rounded)
        if l == 0:
            out["dx"] = dA
            break
        s = f["s16"][l - 1] if saves == "lean" else act_grad(acts[l - 1], f["z"][l - 1], f["y"][l - 1])
        dz = dA * hook("s", l - 1, s)
    return (out, terms) if want_terms else out


# ---------------------------------------------------------------------------------------------- stage bounds
def lin_bound(h, W, b):
    """A-priori bound of an fp32 accumulation of h W^T + b in ANY order, per element: K U32 (sum |h||w| + |b|), K = the number
    of terms (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5); the caller applies C_SUM."""
    return (W.shape[1] + 1) * U32 * (h.abs().double() @ W.abs().double().t() + b.abs().double())


def stage_checks(p, saved, rounded=True, saves="fp32"):
    """F1: [(stage, reference, per-element bound, info)], every layer's fp64 reference evaluated on the kernel's OWN saved
    input of that layer (saved: {x (M, K0), z [l] or None, y [l] (saves='lean': the bf16 copies), s16 [l]} as fp64), so that
    one bf16 operand that rounds the other way does not cascade.
      z{l}   saved pre-activation: C_SUM x lin_bound
      y{l}   no z saved (ReLU, NONE, TANH layers; lean saves): the activation of the reference sum.  The bound is the sum's
             times the activation's Lipschitz constant (1; SiLU 1.1) plus the activation's tolerance (+ 1 bf16 ulp where y
             is stored as bf16)
      a{l}   z saved: the saved y against act(saved z) at the activation's tolerance alone
      s{l}   lean saves: fp16 act'(z): 0.5 x the sum's bound (|SiLU''| <= 0.5) + the tolerance + 1 fp16 ulp"""
    dims, acts = p["dims"], p["acts"]
    L = len(acts)
    out = []
    h = saved["x"]
    for l in range(L):
        Wd, bd = _r(p["W"][l].double(), rounded), p["b"][l].double()
        hr = _r(h, rounded)
        zref, zb = hr @ Wd.t() + bd, C_SUM * lin_bound(hr, Wd, bd)
        a = acts[l]
        lean = saves == "lean" and l + 1 < L
        if saved["z"][l] is not None and not lean:
            out.append((f"z{l}", zref, zb, {}))
            tol, e32 = act_tolerance(a, saved["z"][l])
            out.append((f"a{l}", act(a, saved["z"][l].double()), tol, {"torch32": e32}))
        else:
            tol, e32 = act_tolerance(a, zref)
            yref = act(a, zref)
            bound = (1.1 if a == ACT_SILU else 1.0) * zb + tol
            if lean:
                bound = bound + bf16_ulp(yref)  # (the stored value is the rounding of a value inside the bound: one ulp further at most)
            out.append((f"y{l}", yref, bound, {"torch32": e32}))
            if lean:
                sfn = lambda t: act_grad(a, t, act(a, t))  # noqa: E731
                stol, se32 = act_tolerance(a, zref, sfn)
                sref = sfn(zref)
                out.append((f"s{l}", sref, 0.5 * zb + stol + fp16_ulp(sref), {"torch32": se32}))
        h = saved["y"][l]
    return out


def bound_use(got, ref, bound):
    """Worst |got - ref| / bound over every element (1.0 = at the bound); inf for a non-finite value."""
    got = got.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def pad_rows_zero(save, M):
    """Rows [M, padded(M)) of a bf16 / fp16 save: the many-row weight gradients stream them, so they must be exactly zero."""
    return not bool(save[M:].any())


# ------------------------------------------------------------------------------------------- error measures
def relerr(got, ref):
    """The whole-tensor metric of tests/test_kernels_gpu.py."""
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def per_row_relerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    den = torch.maximum(ref.norm(dim=1), ref.norm() / math.sqrt(ref.shape[0])).clamp_min(1e-300)
    return (got - ref).norm(dim=1) / den


def slice_relerr(got, ref):
    """Worst relative error over the rows (slices) of two (slices, elements) matrices; a slice far below the tensor's typical
    slice is a cancellation whose error scale is the typical slice's, so the denominator is floored at the RMS slice norm
    (encoder_ref.slice_relerr)."""
    return float(per_row_relerr(got, ref).max())


def groups16(v):
    """A bias gradient as (groups, 16) - zero padded."""
    v = v.detach().double().cpu().reshape(-1)
    n = (v.numel() + 15) // 16 * 16
    return F.pad(v, (0, n - v.numel())).reshape(-1, 16)


CLASSES = ["dx/row", "dW/neuron", "db/group16"]


def grad_errors(got, ref):
    """{(class, layer): slice_relerr} of two backward() style dicts (a missing / None entry of `got` is skipped)."""
    out = {}
    if got.get("dx") is not None:
        out[("dx/row", 0)] = slice_relerr(got["dx"], ref["dx"])
    for l, (gw, gb) in enumerate(zip(got["dW"], got["db"])):
        if gw is not None:
            out[("dW/neuron", l)] = slice_relerr(gw, ref["dW"][l])
            out[("db/group16", l)] = slice_relerr(groups16(gb), groups16(ref["db"][l]))
    return out


def class_levels(errors_list):
    lv = {}
    for errs in errors_list:
        for (c, _), e in errs.items():
            lv[c] = max(lv.get(c, 0.0), e)
    return lv


# ------------------------------------------------------------------- references and levels of the GPU tests
# The row counts of tests/test_mlp_fp64_gpu.py: the regime edges themselves (workgroups of 32 / 64 / 128 rows, the switches
# at 2048 and 16384 rows, the padded row count a multiple of 64 or not), per regime.
ROWS_SMALL = [1, 9, 31, 32, 33, 300, 2047]
ROWS_MID = [2048, 2049, 2111, 2112, 4224]
ROWS_HUGE = [16384, 16385, 16461, 33024]
LEVEL_ROWS = {"few": [1, 9, 33], "many": [300, 2112]}  # the problems that pool the oracle's levels (every site)
# (site, rows) of the GPU tests: every regime edge on the Q head (the site the many-row kernels serve), the edges of the
# few-row kernels and of the 2048-row switch of the launch geometry on the others
CASES = {
    "q_head": ROWS_SMALL + ROWS_MID + ROWS_HUGE,
    "q3": [33, 2049, 16385],
    "actor_head": [1, 33, 300, 2049],
    "goal_enc": [9, 31, 32, 33, 300, 2048],
    "goal_enc_tanh": [9, 33, 300, 2047],
    "narrow": [1, 33, 300, 2112],
}

_cache = {}


def reference(site, M, seed=0, saves="fp32"):
    """(problem, forward(), backward(), terms) of the fully rounded fp64 reference, computed once."""
    key = ("ref", site, M, seed, saves)
    if key not in _cache:
        p = problem(site, M, seed)
        x = p["x"][:, :p["dims"][0]]
        f = forward((p["W"], p["b"]), x, p["dims"], p["acts"], saves=saves)
        bw, terms = backward((p["W"], p["b"]), x, p["d_out"], p["dims"], p["acts"], saves=saves, fwd=f, want_terms=True)
        _cache[key] = (p, f, bw, terms)
    return _cache[key]


def oracle_run(O, p, rounded=True, dtype=torch.float32):
    """The oracle's linear layers (oracle.tacorl_oracle, torch autograd) on problem p under bf16 operand rounding in fp32 -
    or without rounding, in `dtype`.  -> (out, backward()-style dict)."""
    L = len(p["acts"])
    W = [w.to(dtype).clone().requires_grad_(True) for w in p["W"]]
    b = [v.to(dtype).clone().requires_grad_(True) for v in p["b"]]
    x = p["x"][:, :p["dims"][0]].to(dtype).clone().requires_grad_(True)
    with O.operand_rounding(torch.bfloat16 if rounded else None):
        h = x
        for l in range(L):
            h = act(p["acts"][l], O._linear(h, W[l], b[l]))
        (h * p["d_out"].to(dtype)).sum().backward()
    return h.detach(), dict(dx=x.grad, dW=[w.grad for w in W], db=[v.grad for v in b])


def oracle_errors(O, site, M, seed=0):
    """(worst per-row output error, grad_errors) of the fp32 rounded oracle against the fp64 rounded reference, same problem."""
    key = ("oracle", site, M, seed)
    if key not in _cache:
        p, f, bw, _ = reference(site, M, seed)
        out, g = oracle_run(O, p)
        _cache[key] = (float(per_row_relerr(out, f["out"]).max()), grad_errors(g, bw))
    return _cache[key]


def bucket(M):
    return "few" if M < 64 else "many"


def levels(O, M):
    """({class: level}, output level) for a problem of M rows: the oracle's worst slice error over the pooled problems of
    M's bucket - every site at LEVEL_ROWS.  What the level measures is a bf16 operand that rounds the other way in fp32
    than in fp64, a chance event per element whose weight in a slice falls with the number of rows that share the slice:
    a class needs enough elements to sample it (encoder_ref.grad_class), and few-row problems are pooled apart from
    many-row ones because one such operand is the whole of a one-row slice."""
    key = ("levels", bucket(M))
    if key not in _cache:
        errs = [oracle_errors(O, s, m) for s in SITES for m in LEVEL_ROWS[bucket(M)]]
        _cache[key] = (class_levels([e[1] for e in errs]), max(e[0] for e in errs))
    return _cache[key]


def grad_bounds(O, site, M, seed=0):
    """{class: GRAD_FACTOR x max(pooled level, the oracle's own error on this problem)} and the same for the output rows."""
    lv, out_lv = levels(O, M)
    own_out, own = oracle_errors(O, site, M, seed)
    own = class_levels([own])
    return ({c: GRAD_FACTOR * max(lv[c], own.get(c, 0.0)) for c in lv}, E2E_FACTOR * max(out_lv, own_out),
            {c: max(lv[c], own.get(c, 0.0)) for c in lv}, max(out_lv, own_out))


ADD_LAMBDA = 4.0


def additivity_bound(terms, kind, l, M, worst_case=False):
    """B3: |grad(A u B) - (grad(A) + grad(B))| per element.  Both sides are fp32 sums of the SAME M terms (a row's dZ does
    not depend on its place in a launch: F3), so they differ by summation order only.
      worst_case: C_SUM M U32 sum |terms| - the a-priori bound of an fp32 sum in any order (Higham eq. 4.4), C_SUM for the two
                  sums compared.  M U32 is 1e-3 at 16461 rows: 16 x the weight of ONE row in the sum, so from ~ 1000 rows on
                  this bound cannot see a dropped row (tests/test_mlp_ref_cpu.py).
      default:    the smaller of that and C_SUM ADD_LAMBDA sqrt(M) U32 sum |terms| - rounding errors of either sign
                  accumulate as sqrt(M), not M: each sum is within lambda sqrt(M) U32 sum |terms| except with probability
                  2 M exp(-lambda^2 / 2) per element under the model of Higham & Mary, A new approach to probabilistic
                  rounding error analysis (SIAM J. Sci. Comput. 41, 2019, thm 2.4), which a sequential sum attains and a
                  blocked one (32-row MFMA steps, slices, a reduce: mlp_fused.hip:583-650) stays far below.  The test
                  asserts this one and records its use of both."""
    wc = C_SUM * M * U32 * terms[kind][l]
    return wc if worst_case else torch.minimum(wc, C_SUM * ADD_LAMBDA * math.sqrt(M) * U32 * terms[kind][l])


def accumulate_bound(total):
    """accumulate = 1: base + grad is ONE fp32 rounding of the sum (encoder_ref.accumulate_rounding), per element."""
    return 2 * U32 * total.abs().double()
