"""fp64 restatement of the ring GEMM and of its weight gradients (tacorl_amd/csrc/rnn_ops.hip), the launcher rules that pick
a tile template and a workgroup map, seeded problems that make the checks discriminating, the a-priori bounds of an fp32
accumulation and the shape tables tests/test_ring_fp64_gpu.py runs (tests/test_ring_ref_cpu.py shows what the bounds still
detect and that the tables reach every template).  Plain torch on the CPU: no GPU, no kernel of this repository.

Rounding points, read from rnn_gemm_kernel (every rounding is round-to-nearest-even):
  x, W, x_ext, w_ext   bf16 as given, staged by LDS-DMA and multiplied by the MFMA into an fp32 accumulator that starts at +0:
                       K / 128 main tiles in order (none when x == NULL), then the extension tile
  z                    acc + bias, + bias2, + addend, in that order, each an fp32 addition (epilogue `z += ...`)
  y                    act_apply(act, z) in fp32, then `ms > 0.f ? z : 0.f` on the mask source (not for twin rows:
                       `if (a.mask_src && !twin)`); +0.0 and -0.0 in the mask source both gate to 0
  bf16 copy            `(__bf16)z[r]` of the fp32 y
and from rnn_wgrad_body: dW = dz^T x over R rows in 32-row MFMA steps into fp32, db = the same MFMA against ones (column sums
of the bf16 dz), accumulate = 1: one fp32 addition of what the destination held; the slabs form sums the slabs' partial
results in slab order (wgrad_slab_sum_kernel), starting from the destination (accumulate) or +0."""
import torch

from tests import mlp_ref as MR

ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH = MR.ACT_NONE, MR.ACT_RELU, MR.ACT_SILU, MR.ACT_TANH
U32, C_SUM, ACT_FACTOR, FAULT_RATIO = MR.U32, MR.C_SUM, MR.ACT_FACTOR, MR.FAULT_RATIO
GATE_CAP = 0.01          # ReLU gates whose |z| lies within the bound of zero: below this share of the output
RB_K = 128               # rnn_ops.hip RB_K: columns of a K tile, and the width of the K extension
WG_T, WG_RMIN = 128, 64  # rnn_ops.hip: edge of a weight-gradient tile, reduction rows per stage
GUARD = 4                # NaN rows in front of and behind every operand (4 rows of any legal pitch keep 16-byte alignment)
NAN = float("nan")

# tile template -> (RB_M, RB_N, RB_S, waves): every instantiation of rnn_gemm_kernel in rnn_ops.hip
TEMPLATES = {"64x32/4": (64, 32, 4, 4), "64x32/2": (64, 32, 2, 4), "64x64/3": (64, 64, 3, 4), "128x64/3": (128, 64, 3, 4),
             "128x64/2": (128, 64, 2, 8), "128x128/2": (128, 128, 2, 8)}


# ------------------------------------------------------------------------------------------------- launcher rules
def _small(nprob, rows, N):
    """launch_small: 64 x 32 tiles, the 4-stage ring while the launch is at most 192 workgroups."""
    MT, NTX = (rows + 63) // 64, (N // 32 + 7) // 8
    return ("64x32/4" if 8 * MT * NTX * nprob <= 192 else "64x32/2", "xcd")


def route(entry, nprob, M, M2, K, N):
    """(tile template, workgroup map) of a launch, by the rules of tacorl_rnn_linear_fwd ("fwd"), tacorl_rnn_linear_bwd_step
    ("bwd_step"), rnn_fwd_batch ("fwd_batch", "twin", "ext"), tacorl_rnn_linear_bwd_batch ("bwd_batch"), tacorl_rnn_linear_ld
    ("ld") and launch_small, as rnn_ops.hip states them."""
    assert K >= RB_K and K % RB_K == 0 and N >= 32 and N % 32 == 0 and M >= 1, "tacorl_rnn_linear_supported"
    big = M * N >= 256 * 64 * 128 and N % 64 == 0
    if entry == "fwd":
        if big:
            return ("128x64/3", "xcd")
        if N % 64 == 0 and N // 64 < 8 and M >= 1024:
            return ("64x64/3", "plain")
        return ("64x32/4", "xcd")
    if entry == "bwd_step":
        return ("64x32/4", "xcd")
    if entry == "ld":
        return ("128x64/3", "xcd") if big else _small(nprob, M, N)
    assert entry in ("fwd_batch", "twin", "ext", "bwd_batch"), entry
    rows = M + M2  # (tile choice: by the rows of the launch)
    if nprob <= 2 and rows % 64 == 0:
        return _small(nprob, rows, N)
    if entry != "bwd_batch" and M2 > 0 and nprob > 2 and rows >= 512 and rows % 128 == 0 and N % 128 == 0:
        return ("128x128/2", "xcd")
    if rows % 128 == 0 and N % 64 == 0:
        return ("128x64/2", "xcd")
    return _small(nprob, rows, N)


def wgrad_map(M, N):
    """rnn_wgrad_body's tile map: an XCD owns a block of MT / 4 x NT / 2 tiles where that divides, one tile per block index
    otherwise."""
    MT, NT = M // WG_T, N // WG_T
    return "xcd-block" if MT % 4 == 0 and NT % 2 == 0 else "plain"


def ring_steps(K, ext=False, x_null=False):
    """nk of rnn_gemm_kernel: main K tiles (none for a NULL operand) plus the extension tile."""
    return (0 if x_null else K // RB_K) + (1 if ext else 0)


def idle_tiles(tile, N):
    """Workgroups of the XCD map that return early: 8 NTX - NT per M tile and problem."""
    NT = N // TEMPLATES[tile][1]
    return 8 * ((NT + 7) // 8) - NT


# ------------------------------------------------------------------------------------------------------ rounding
def bf(t):
    return t.to(torch.bfloat16)


def bf16_trunc(y):
    """A bf16 copy made by dropping the low 16 bits of the fp32 value (the fault of tests/test_ring_ref_cpu.py)."""
    return (y.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- restatement
def linear(p, dtype=torch.float64, twin=False):
    """z = x W^T + x_ext w_ext^T + b + b2 + addend of problem p (its twin rows: x2, x2_ext, addend2) in `dtype`, the additions
    in the kernel's order.  -> {z, mag: sum of the magnitudes of every term, n: number of terms, gate: bool or None}."""
    x, xe, ad = (p.get("x2"), p.get("xe2"), p.get("ad2")) if twin else (p.get("x"), p.get("xe"), p.get("ad"))
    rows = p["M2"] if twin else p["M"]
    w = p["w"]
    N = w.shape[0]
    z, mag, n = torch.zeros(rows, N, dtype=dtype), torch.zeros(rows, N, dtype=torch.float64), 0
    if x is not None:
        z = z + x.to(dtype) @ w.to(dtype).t()
        mag += x.double().abs() @ w.double().abs().t()
        n += w.shape[1]
    if xe is not None:
        z = z + xe.to(dtype) @ p["we"].to(dtype).t()
        mag += xe.double().abs() @ p["we"].double().abs().t()
        n += RB_K
    for t in (p.get("b"), p.get("b2"), ad):
        if t is not None:
            z = z + t.to(dtype)
            mag += t.double().abs()
            n += 1
    ms = None if twin else p.get("mask")
    return dict(z=z, mag=mag, n=n, gate=None if ms is None else ms > 0)


def output(r, act):
    """y = act(z) [mask_src > 0] of a linear() result."""
    y = MR.act(act, r["z"])
    return y if r["gate"] is None else torch.where(r["gate"], y, torch.zeros_like(y))


def bound(r, act):
    """Per-element bound of the kernel's fp32 y against output(linear(p), act) in fp64, and the number of undecidable gates.
    The sum: C_SUM n U32 (sum |x||w| + |b| + |b2| + |addend|) - an fp32 accumulation of n terms in any order (Higham, Accuracy
    and Stability of Numerical Algorithms, eq. 3.5).  ReLU is exact given z and 1-Lipschitz: the same bound; a gate whose |z|
    is within it may go either way and is counted.  SiLU (Lipschitz 1.1) and Tanh add ACT_FACTOR x plain fp32 torch's error
    on the same z (mlp_ref.act_tolerance).  The mask is exact: a masked element must be 0, bound 0."""
    zb = C_SUM * r["n"] * U32 * r["mag"]
    b, ties = zb, 0
    if act == ACT_RELU:
        open_ = torch.ones_like(zb, dtype=torch.bool) if r["gate"] is None else r["gate"]
        ties = int(((r["z"].double().abs() <= zb) & open_).sum())
    elif act in (ACT_SILU, ACT_TANH):
        tol, _ = MR.act_tolerance(act, r["z"].double())
        b = (1.1 if act == ACT_SILU else 1.0) * zb + tol
    if r["gate"] is not None:
        b = torch.where(r["gate"], b, torch.zeros_like(b))
    return b, ties


def use(got, ref, bnd):
    """Worst |got - ref| / bound; inf for a non-finite value or an error where the bound is 0."""
    got = got.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref.double()).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300))
    return float(q.max()) if q.numel() else 0.0


def copy_bound(ref, bnd):
    """A bf16 copy that has no fp32 twin to be compared with bit for bit (y == NULL): the rounding of a value inside the
    bound - one bf16 ulp further at most."""
    return bnd + MR.bf16_ulp(ref)


def wgrad(dz, x, dtype=torch.float64):
    """{dW (M, N), db (M), magW, magb} of dW = dz^T x, db = column sums of dz (bf16 operands as given)."""
    d, v = dz.to(dtype), x.to(dtype)
    return dict(dW=d.t() @ v, db=d.sum(0), magW=dz.double().abs().t() @ x.double().abs(), magb=dz.double().abs().sum(0))


def wgrad_bound(mag, R):
    """C_SUM R U32 sum |dz||x|: an fp32 sum of R terms in any order."""
    return C_SUM * R * U32 * mag


def accumulate_bound(bnd, total):
    """accumulate = 1: one fp32 rounding of base + grad on top of the gradient's own bound."""
    return bnd * (1 + U32) + U32 * total.double().abs()


# ------------------------------------------------------------------------------------------------------- problems
def _g(seed):
    return torch.Generator().manual_seed(seed)


def problem(M, K, N, seed, bias=True, bias2=False, addend=True, ext=0, mask=False, x_null=False, M2=0):
    """One seeded problem: x (M, K) ~ N(0, 1) and w (N, K) ~ N(0, 1) / sqrt(K) in bf16, biases N(0, 0.5), addend N(0, 1);
    ext > 0: the K extension with `ext` real columns, x_ext (M, 128) and w_ext (N, 128) zero padded (contract); mask: a mask
    source with exact +0.0 and -0.0 entries; x_null: no main operand (x = None); M2 > 0: twin rows x2, addend2 (x_ext2)."""
    g = _g(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = dict(M=M, M2=M2, K=K, N=N, ext=ext)
    x = bf(rn(M, K))
    p["x"] = None if x_null else x
    p["w"] = bf(rn(N, K) / K ** 0.5)
    p["b"] = rn(N) * 0.5 if bias else None
    p["b2"] = rn(N) * 0.5 if bias2 else None
    p["ad"] = rn(M, N) if addend else None
    if ext:
        pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], RB_K - ext, dtype=t.dtype)], 1).contiguous()  # noqa: E731
        p["xe"], p["we"] = pad(bf(rn(M, ext))), pad(bf(rn(N, ext) / ext ** 0.5))
    if mask:
        ms = rn(M, N)
        ms.view(-1)[::7] = 0.0
        ms.view(-1)[3::11] = -0.0
        p["mask"] = ms
    if M2:
        p["x2"] = bf(rn(M2, K))
        p["ad2"] = rn(M2, N) if addend else None
        if ext:
            p["xe2"] = pad(bf(rn(M2, ext)))
    return p


def padded(t, ld=None, guard=GUARD, fill=NAN, col=0):
    """t (rows, cols) as the column slice [col, col + cols) of a (rows + 2 guard, ld) buffer of NaN: what the kernel must not
    read.  -> (whole, the view that starts at the slice's first element)."""
    ld = ld or t.shape[1] + col
    whole = torch.full((t.shape[0] + 2 * guard, ld), fill, dtype=t.dtype)
    whole[guard: guard + t.shape[0], col: col + t.shape[1]] = t
    return whole, whole[guard: guard + t.shape[0], col:]


def wgrad_problem(R, M, N, seed, rows=None):
    """dz (R, M) ~ N(0, 1) + 0.25 (a mean: the bias sums are no cancellations) and x (R, N) ~ N(0, 1) in bf16; rows: the slabs
    form's real output rows - columns [rows, M) of dz hold zeros (contract)."""
    g = _g(seed)
    dz, x = bf(torch.randn(R, M, generator=g) + 0.25), bf(torch.randn(R, N, generator=g))
    if rows is not None:
        dz[:, rows:] = 0
    return dict(R=R, M=M, N=N, dz=dz, x=x)


def base(shape, seed):
    """What an accumulating call finds in its destination."""
    return torch.randn(*shape, generator=_g(seed))


# --------------------------------------------------------------------------------------------------- shape tables
ACTS = [ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH]
# G1: tacorl_rnn_linear_fwd (M, K, N) -> the route it is here for
G1 = {(70, 128, 96): ("64x32/4", "xcd"), (100, 640, 288): ("64x32/4", "xcd"), (1030, 384, 192): ("64x64/3", "plain"),
      (4100, 512, 512): ("128x64/3", "xcd"), (3700, 128, 576): ("128x64/3", "xcd")}
G1_BWD_STEP = (37, 256, 160)
# G2: (entry, nprob, M, M2, K, N, extension widths per problem or None) -> tile.  The extension rides on a subset of problems,
# real width 40 and 128; "null": that problem's x is NULL (zero operand) - only without twin rows
G2 = {
    ("fwd_batch", 1, 64, 0, 128, 96, None): "64x32/4",
    ("fwd_batch", 2, 448, 0, 384, 288, None): "64x32/2",
    ("fwd_batch", 4, 200, 0, 384, 288, None): "64x32/2",
    ("fwd_batch", 3, 70, 0, 256, 96, None): "64x32/4",
    ("fwd_batch", 3, 128, 0, 384, 192, None): "128x64/2",
    ("fwd_batch", 4, 128, 0, 384, 192, None): "128x64/2",
    ("twin", 3, 300, 212, 384, 128, None): "128x128/2",
    ("twin", 1, 40, 24, 256, 64, None): "64x32/4",
    ("ext", 3, 70, 0, 256, 96, (40, 0, 128)): "64x32/4",
    ("ext", 2, 448, 0, 640, 288, (0, 128)): "64x32/2",
    ("ext", 4, 128, 0, 384, 192, ("null40", 128, 0, "null128")): "128x64/2",
    ("ext", 3, 300, 212, 384, 128, (40, 128, 0)): "128x128/2",
    ("ext", 1, 64, 0, 128, 96, ("null40",)): "64x32/4",
}
# G3: tacorl_rnn_linear_ld (nprob, M, K, N, ldx, ldy)
G3 = {(2, 24, 128, 64, 256, 192): "64x32/4", (2, 4100, 128, 512, 136, 1024): "128x64/3"}
# W1: tacorl_rnn_wgrad
W1_R = [64, 128, 320]
W1_MN = {(128, 128): "plain", (384, 128): "plain", (256, 384): "plain", (512, 256): "xcd-block", (512, 512): "xcd-block"}
W2_R = [64, 192, 128, 320]
W2_MN = [(128, 128), (512, 256)]
# W3: tacorl_rnn_wgrad_slabs (R, slabs, rows, Mp, N)
W3 = [(128, 1, 128, 128, 128), (384, 3, 100, 128, 256), (512, 2, 182, 256, 256)]


def ext_spec(e):
    """An entry of G2's extension tuple -> (real width or 0, x is NULL)."""
    if isinstance(e, str):
        return int(e[4:]), True
    return int(e or 0), False


def g2_problems(key):
    """The problems of a G2 launch.  Optional operands rotate over the problems as COMBOS does in
    tests/test_action_decoder_gpu.py: problem p has an addend unless p % 3 == 1; the GPU test gives it a bf16 copy unless
    p % 3 == 1 and no fp32 output (y == NULL, the copy alone) where p % 3 == 2.  act rotates ReLU, none, SiLU, Tanh."""
    entry, nprob, M, M2, K, N, ext = key
    out = []
    for p in range(nprob):
        w, nul = ext_spec(ext[p]) if ext else (0, False)
        q = problem(M, K, N, seed=1000 + 17 * p + M + K + N, bias=True, bias2=w > 0 and p != 1, addend=p % 3 != 1, ext=w,
                    x_null=nul, M2=M2)
        q["act"] = [ACT_RELU, ACT_NONE, ACT_SILU, ACT_TANH][p]
        out.append(q)
    return out


def g3_problems(key):
    """The two problems of a G3 launch: bias and the extension (40 real columns) in the first, bias2 and the addend in the
    second, a mask source in both."""
    nprob, M, K, N, _, _ = key
    return [problem(M, K, N, seed=M + N, bias=True, addend=False, ext=40, mask=True),
            problem(M, K, N, seed=M + N + 1, bias=False, bias2=True, addend=True, mask=True)]


def ring_cases():
    """Every ring launch of the tables as (entry, nprob, M, M2, K, N, nk of each problem)."""
    out = [("fwd", 1, M, 0, K, N, [ring_steps(K)]) for (M, K, N) in G1]
    M, K, N = G1_BWD_STEP
    out.append(("bwd_step", 1, M, 0, K, N, [ring_steps(K)]))
    for (entry, nprob, M, M2, K, N, ext) in G2:
        specs = [ext_spec(e) for e in (ext or [0] * nprob)]
        out.append((entry, nprob, M, M2, K, N, [ring_steps(K, w > 0, nul) for w, nul in specs]))
    for (nprob, M, K, N, _, _) in G3:
        out.append(("ld", nprob, M, 0, K, N, [ring_steps(K, True), ring_steps(K)]))
    return out
