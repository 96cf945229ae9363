"""The fused MLP chain (tacorl_amd/csrc/mlp_fused.hip: few-row, 32-row many-row, 128 / 64-row and persistent kernels; lean
saves, gathered input, batched preparation and reduces) and the per-layer path of dense_ops.hip per row, per layer and per
neuron against the fp64 restatement of tests/mlp_ref.py, at the row counts where the kernels change: the workgroup sizes
32 / 64 / 128, the regime switches at 2048 and 16384 rows, ragged ends, the persistent loop's stride.

  F1  every saved z, y, bf16 y, fp16 act' and the output, element by element, against the fp64 stage evaluated on the
      kernel's own saved input: |got - ref| <= 2 K 2^-24 (sum |x||w| + |b|) (+ 1 bf16 / fp16 ulp where stored so); act(z) at
      4 x plain fp32 torch's error on the same z; pad rows of the bf16 / fp16 saves zero, gaps and skipped regions still NaN
  F2  every output row against the fully rounded reference, at 4 x the fp32 rounded oracle's worst row
  F3  the same rows at several places of a launch and in either problem: bit-identical; the gathered forward equals the
      plain one bit for bit, pad columns of x_out zero
  B1  d_x per row, B2 dW per output neuron and db per 16 elements of every layer, at 4 x the oracle's error on the slice
      class; accumulate = 1 is base + grad up to one fp32 rounding; prep_batch / reduce_batch equal the plain calls
  B3  the gradients of a problem equal the sum of its two row-halves' up to the fp32 sum's bound
  B4  refusals come before any launch

Every bound comes from tests/mlp_ref.py (tests/test_mlp_ref_cpu.py shows what the bounds still detect); every measured
number goes to golden_util.record_margin (tools/mlp_margins_md.py -> profiles/mlp_margins.md).  A test collects all its
figures before it asserts."""
import ctypes as C

import pytest
import torch

from tests import mlp_ref as R
from tests.golden_util import record_margin

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
NAN = float("nan")


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _flat(p, dev):
    """The fp32 parameter block of problem p and its bf16 mirror."""
    from tacorl_amd import blocks

    dims, L = p["dims"], len(p["acts"])
    flat = torch.zeros(blocks.mlp_size(dims), device=dev)
    v = blocks.mlp_views(flat, 0, dims, [(f"w{l}", f"b{l}") for l in range(L)])
    for l in range(L):
        v[f"w{l}"].copy_(p["W"][l])
        v[f"b{l}"].copy_(p["b"][l])
    return flat, flat.to(torch.bfloat16)


def _grad_views(g, dims):
    from tacorl_amd import blocks

    L = len(dims) - 1
    v = blocks.mlp_views(g, 0, dims, [(f"w{l}", f"b{l}") for l in range(L)])
    return dict(dW=[v[f"w{l}"] for l in range(L)], db=[v[f"b{l}"] for l in range(L)])


def _second(site, M, mode):
    """The second problem of a call: 130 rows (a few-row problem beside a many-row one exercises the lean-site split of
    mlp_fwd_fused_impl), or - mode 'two' - M - 4000 rows: two many-row problems halve the persistent kernels' grid, so
    that every workgroup runs its block loop more than once."""
    return R.reference(site, M - 4000 if mode == "two" else 130, seed=1)


class _Call:
    """One (path, site, rows, mode) call: its problems on the device and what the kernels left behind."""

    def __init__(self, path, site, M, mode, monkeypatch):
        self.dev = _dev()
        self.path, self.site, self.mode = path, site, mode
        self.lean = path in ("lean", "lean_pers0")
        self.compute = 0 if path == "layer_f32" else 1
        self.refs = [R.reference(site, M)] + ([_second(site, M, mode)] if mode != "one" else [])
        self.probs = [r[0] for r in self.refs]
        self.Ms = [p["M"] for p in self.probs]
        p = self.probs[0]
        self.dims, self.acts, self.ld, self.L = p["dims"], p["acts"], p["ld"], len(p["acts"])
        self.many = [self.lean and R.regime(site, m) != "small" for m in self.Ms]
        pers = "0" if path == "lean_pers0" else "1"
        monkeypatch.setenv("TACORL_MLP_PERS", pers)
        monkeypatch.setenv("TACORL_MLP_PERS_BWD", pers)
        self.xs = [q["x"].to(self.dev) for q in self.probs]
        fl = [_flat(q, self.dev) for q in self.probs]
        self.flats, self.fb = [f[0] for f in fl], [f[1] for f in fl]
        self.douts = [q["d_out"].to(self.dev).contiguous() for q in self.probs]
        self.tag = f"t_mlp64_{path}_{site}_{M}_{mode}"

    def alone(self, i, path):
        """Problem i of this call as a call of its own on `path` (the same device tensors)."""
        c = _Call.__new__(_Call)
        c.__dict__.update(self.__dict__)
        c.path, c.mode, c.lean = path, "one", path in ("lean", "lean_pers0")
        c.refs, c.probs, c.Ms = [self.refs[i]], [self.probs[i]], [self.Ms[i]]
        c.xs, c.flats, c.fb, c.douts = [self.xs[i]], [self.flats[i]], [self.fb[i]], [self.douts[i]]
        c.many = [c.lean and R.regime(self.site, m) != "small" for m in c.Ms]
        return c

    def forward(self):
        from tacorl_amd import _lib, ops

        self.bufs = [torch.full((ops.mlp_act_layout(m, self.dims, self.acts)[2],), NAN, device=self.dev) for m in self.Ms]
        if self.path.startswith("layer"):
            ops.mlp_fwd(self.xs, self.ld, self.flats, self.bufs, self.Ms, self.dims, self.acts, self.compute)
        else:
            assert _lib.lib().tacorl_mlp_fwd_fused_supported(len(self.Ms), self.L, ops.int_array(self.dims), self.ld) == 1
            if self.lean:
                assert ops.mlp_lean_ok(len(self.Ms), self.dims, self.ld, self.dims[-1], self.ld, 1)
            ops.mlp_fwd(self.xs, self.ld, self.flats, self.bufs, self.Ms, self.dims, self.acts, 1, params_bf16=self.fb, lean=self.lean)
        torch.cuda.synchronize()
        return self

    def saved(self, i):
        """-> (got {stage: fp64 cpu tensor}, saved dict for mlp_ref.stage_checks, pad rows zero?, untouched floats still NaN?)"""
        from tacorl_amd import ops

        M, dims, acts, L, buf = self.Ms[i], self.dims, self.acts, self.L, self.bufs[i]
        zo, yo, tot = ops.mlp_act_layout(M, dims, acts)
        Mp = R.padded(M)
        written = torch.zeros(tot, dtype=torch.bool, device=buf.device)
        got, sv, pads_zero = {}, dict(x=self.probs[i]["x"][:, :dims[0]].double(), z=[None] * L, y=[None] * L), True
        for l in range(L):
            N = dims[l + 1]
            if self.many[i] and l + 1 < L:  # bf16 y [Mp][N] in the y region, fp16 act' [Mp][N] in the z region
                n2 = Mp * N // 2
                yb = buf[yo[l]: yo[l] + n2].view(torch.bfloat16).view(Mp, N)
                sb = buf[zo[l]: zo[l] + n2].view(torch.float16).view(Mp, N)
                written[yo[l]: yo[l] + n2] = True
                written[zo[l]: zo[l] + n2] = True
                pads_zero = pads_zero and R.pad_rows_zero(yb, M) and R.pad_rows_zero(sb, M)
                sv["y"][l] = got[f"y{l}"] = yb[:M].double().cpu()
                got[f"s{l}"] = sb[:M].double().cpu()
                continue
            if zo[l] >= 0:
                sv["z"][l] = got[f"z{l}"] = buf[zo[l]: zo[l] + M * N].view(M, N).double().cpu()
                written[zo[l]: zo[l] + M * N] = True
            if self.lean and l + 1 < L and zo[l] >= 0:  # few-row lean: a hidden SiLU layer's output is not saved
                continue
            sv["y"][l] = got[f"y{l}"] = got[f"a{l}"] = buf[yo[l]: yo[l] + M * N].view(M, N).double().cpu()
            written[yo[l]: yo[l] + M * N] = True
        gaps_nan = bool(torch.isnan(buf[~written]).all())
        return got, sv, pads_zero, gaps_nan

    def backward(self, want_dx, no_grads=(), accumulate=False, base=None):
        """-> (d_x list or None, gradient blocks); base: what the blocks hold before an accumulating call."""
        from tacorl_amd import ops

        n = len(self.Ms)
        dx = [torch.full((m, self.ld), NAN, device=self.dev) for m in self.Ms] if want_dx else None
        gr = [None if i in no_grads else (torch.full_like(self.flats[i], NAN) if base is None else base[i].clone()) for i in range(n)]
        NL = self.dims[-1]
        if self.path.startswith("layer"):
            ops.mlp_bwd(self.xs, self.ld, self.flats, self.bufs, self.douts, NL, gr, dx, self.ld, self.Ms, self.dims, self.acts,
                        self.compute, accumulate=accumulate, ws_tag=self.tag)
        else:
            assert ops.mlp_bwd_fused_ok(n, self.dims, NL, self.ld, 1)
            ops.mlp_bwd_fused_dgrad(self.flats, self.bufs, self.douts, NL, dx, self.ld, self.Ms, self.dims, self.acts, self.tag, lean=self.lean)
            ops.mlp_bwd_fused_wgrad(self.xs, self.ld, self.bufs, self.douts, NL, gr, self.Ms, self.dims, self.acts, self.tag,
                                    accumulate=accumulate, lean=self.lean)
        torch.cuda.synchronize()
        return dx, gr


# ================================================================================================== cases
def _cases():
    """(path, site, rows, mode): every (site, rows) of mlp_ref.CASES with everything saved ('save': the few-row kernel,
    128 / 64-row workgroups from 2048 rows on) and lean ('lean': the many-row kernels where the site has them) in a mixed
    two-problem call; the huge row counts also alone, with a second many-row problem and on the per-block kernels
    (TACORL_MLP_PERS = TACORL_MLP_PERS_BWD = 0); the per-layer path in bf16 and f32."""
    out = []
    for site, rows in R.CASES.items():
        for M in rows:
            out += [("save", site, M, "mixed"), ("lean", site, M, "mixed")]
    out += [("lean", "q_head", 16461, "one"), ("lean", "q_head", 16461, "two"), ("lean", "q_head", 16384, "one"), ("lean", "q3", 16385, "two"),
            ("lean_pers0", "q_head", 16384, "mixed"), ("lean_pers0", "q_head", 16461, "mixed"), ("lean_pers0", "q3", 16385, "mixed")]
    for site, M in (("q_head", 300), ("goal_enc_tanh", 33), ("narrow", 2112), ("actor_head", 33)):
        out += [("layer_bf16", site, M, "mixed"), ("layer_f32", site, M, "mixed")]
    return out


CASES = _cases()
IDS = ["-".join(str(v) for v in c) for c in CASES]


# ================================================================================================ F1 / F2
@pytest.mark.parametrize("path,site,M,mode", CASES, ids=IDS)
def test_forward_stage_by_stage_and_per_row(path, site, M, mode, monkeypatch):
    from oracle import tacorl_oracle as O

    c = _Call(path, site, M, mode, monkeypatch).forward()
    rounded = path != "layer_f32"
    worst, act32, bad = {}, {}, []
    for i, (p, f, _, _) in enumerate(c.refs):
        got, sv, pads_zero, gaps_nan = c.saved(i)
        if not pads_zero:
            bad.append((i, "rows behind M of a bf16 / fp16 save are not zero"))
        if not gaps_nan:
            bad.append((i, "a float outside the saved regions was written"))
        if c.lean and not c.many[i] and any(a == R.ACT_SILU for a in c.acts[:-1]):
            # few-row lean: the hidden outputs are skipped, so no stage has its own input - the saved z and the output must be
            # the saving mode's bit for bit (the same kernel, two stores fewer), which the 'save' case checks stage by stage
            g2 = c.alone(i, "save").forward().saved(0)[0]
            for k in got:
                if not torch.equal(got[k], g2[k]):
                    bad.append((i, k, "differs from the saving mode"))
            continue
        for stage, ref, bound, info in R.stage_checks(p, sv, rounded=rounded, saves="lean" if c.many[i] else "fp32"):
            use = R.bound_use(got[stage], ref, bound)
            worst[stage] = max(worst.get(stage, 0.0), use)
            if "torch32" in info:
                act32[stage] = max(act32.get(stage, 0.0), info["torch32"])
            if not use <= 1.0:
                bad.append((i, stage, use))
        if rounded:
            ob, level = R.grad_bounds(O, site, c.Ms[i], seed=i)[1::2]
            e = float(R.per_row_relerr(got[f"y{c.L - 1}"], f["out"]).max())
            worst["rows"] = max(worst.get("rows", 0.0), e / ob)
            record_margin(f"{path} {site} {M} {mode} p{i} rows", e, ob, floor=level, kind="F2 per row")
            if not e <= ob:
                bad.append((i, "per-row output", e, ob))
    tag = f"{path} {site} {M} {mode}"
    print(f"{tag}: err / bound " + ", ".join(f"{s} {u:.3g}" for s, u in worst.items()))
    for s, u in worst.items():
        if s != "rows":
            record_margin(f"{tag} {s}", u, 1.0, floor=act32.get(s), kind="F1 err / bound")
    assert not bad, bad


# ===================================================================================================== F3
@pytest.mark.parametrize("site,M,lean", [("q_head", 300, False), ("goal_enc_tanh", 300, False), ("q_head", 2112 + 45, True),
                                         ("q_head", 16461, True), ("q3", 16385, True)])
def test_forward_same_rows_same_bits_wherever_they_are_served(site, M, lean, monkeypatch):
    """40 probe rows at the start of a launch, across a workgroup boundary (rows 108 .. 147: 128 is a boundary of the 32-,
    64- and 128-row workgroups), at the ragged end, and in a second problem with the same weights: outputs and every save
    of those rows are bit-identical.  (At >= 16384 rows the persistent kernels serve the places from different
    workgroups and loop iterations.)"""
    c = _Call("lean" if lean else "save", site, M, "one", monkeypatch)
    K0, n = c.dims[0], 40
    probe = R.rows(site, n, seed=2).to(c.dev)
    M1 = M - 100 if lean else 200  # (the second problem of a many-row call is a many-row problem too: the same kernel)
    places = [(0, 0), (0, 108), (0, M - n), (1, 50)]
    x1 = torch.full((M1, c.ld), R.PAD, device=c.dev)
    x1[:, :K0] = R.rows(site, M1, seed=1).to(c.dev)
    c.xs, c.Ms = [c.xs[0].clone(), x1], [M, M1]
    c.flats, c.fb, c.probs = c.flats * 2, c.fb * 2, c.probs * 2
    c.many = [lean and R.regime(site, m) != "small" for m in c.Ms]
    assert c.many[0] == c.many[1]
    for pi, r0 in places:
        c.xs[pi][r0: r0 + n, :K0] = probe
    c.forward()
    first, bad = None, []
    for pi, r0 in places:
        got = c.saved(pi)[0]
        here = {k: v[r0: r0 + n] for k, v in got.items()}
        if first is None:
            first = here
            assert all(torch.isfinite(v).all() for v in first.values())
        bad += [(pi, r0, k, int((here[k] != first[k]).sum())) for k in here if not torch.equal(here[k], first[k])]
    assert not bad, bad


@pytest.mark.parametrize("B,lean", [(37, False), (210, True), (1700, True)])
def test_gathered_forward_equals_the_plain_one(B, lean, monkeypatch):
    """tacorl_mlp_fwd_fused_gather on the Q head at 370, 2100 and 17000 rows: the state columns repeat every B rows
    (seg_mod), the action segment is ragged (7 of 8 columns) - bit for bit the buffers of the plain forward on the
    assembled rows (which F1 checks), the assembled copy equals them and its pad column is zero."""
    from tacorl_amd import ops

    site, rep = "q_head", 10
    M = rep * B
    c = _Call("lean" if lean else "save", site, M, "one", monkeypatch)
    dev = c.dev
    state = torch.full((B + 5, 64), NAN, device=dev)
    state[5:] = R.rows(site, B, seed=3)[:, :64].to(dev)
    action = torch.full((M, 8), 3.0, device=dev)
    action[:, :7] = R.rows(site, M, seed=4)[:, 64:71].to(dev)
    x = torch.full((M, c.ld), R.PAD, device=dev)
    x[:, :64] = state[5:][torch.arange(M, device=dev) % B]
    x[:, 64:71] = action[:, :7]
    c.xs = [x]
    c.forward()
    plain = c.bufs[0].clone()
    assert ops.mlp_fwd_gather_ok([M], c.dims, c.acts, c.ld, 1, lean)
    got = torch.full_like(plain, NAN)
    x_out = torch.full((M, c.ld), NAN, device=dev)
    ops.mlp_fwd_gather([[(state, 5 * 64, 64, 0, B), (action, 0, 8, 64, 0)]], [x_out], c.ld, c.flats, c.fb, [got], [M], c.dims, c.acts, lean=lean)
    torch.cuda.synchronize()
    same = torch.equal(got.view(torch.int32), plain.view(torch.int32))
    rows_ok = torch.equal(x_out[:, :71], x[:, :71])
    pad_ok = bool((x_out[:, 71:] == 0).all())
    # ... and the plain buffers are right: F1 on the assembled rows
    p = dict(c.probs[0], x=x.cpu())
    c.probs = [p]
    g, sv, pads_zero, gaps_nan = c.saved(0)
    uses = {}
    if not (lean and not c.many[0]):
        uses = {s: R.bound_use(g[s], ref, b) for s, ref, b, _ in R.stage_checks(p, sv, saves="lean" if c.many[0] else "fp32")}
    print(f"gather {M} rows: bit-identical {same}, err / bound {uses}")
    assert same and rows_ok and pad_ok and pads_zero and gaps_nan
    assert all(u <= 1.0 for u in uses.values()), uses


# ================================================================================================ B1 / B2
_bwd = {}


def _backward_figures(path, site, M, mode, monkeypatch):
    """One backward per case, shared by B1 and B2: d_x wanted unless rows % 4 == 0 (the chain then stops a layer early), the
    second problem without parameter gradients when rows is odd (the actor's pass through the Q networks), then the same
    call with accumulate = 1 on a seeded base."""
    from oracle import tacorl_oracle as O

    key = (path, site, M, mode)
    if key in _bwd:
        return _bwd[key]
    c = _Call(path, site, M, mode, monkeypatch).forward()
    want_dx = M % 4 != 0
    no_grads = (1,) if (M % 2 == 1 and len(c.Ms) > 1) else ()
    dx, gr = c.backward(want_dx, no_grads)
    base = [R.accumulate_base(f.numel(), 900 + i).to(c.dev) for i, f in enumerate(c.flats)]
    _, ga = c.backward(False, no_grads, accumulate=True, base=base)
    rounded = path != "layer_f32"
    fig = dict(errs=[], bounds=[], levels=[], acc=[], finite=True)
    for i, (p, f, bw, _) in enumerate(c.refs):
        if c.many[i]:  # the many-row chain multiplies by the fp16 act' of the lean saves
            p, f, bw, _ = R.reference(site, c.Ms[i], seed=i, saves="lean")
        if not rounded:
            xx = p["x"][:, :c.dims[0]]
            bw = R.backward((p["W"], p["b"]), xx, p["d_out"], c.dims, c.acts, rounded=False)
        got = dict(dx=None, dW=[None] * c.L, db=[None] * c.L)
        if dx is not None:
            got["dx"] = dx[i][:, :c.dims[0]].double().cpu()
            fig["finite"] = fig["finite"] and bool(torch.isfinite(got["dx"]).all())
        if gr[i] is not None:
            v = _grad_views(gr[i], c.dims)
            got["dW"], got["db"] = [t.double().cpu() for t in v["dW"]], [t.double().cpu() for t in v["db"]]
            fig["finite"] = fig["finite"] and all(bool(torch.isfinite(t).all()) for t in got["dW"] + got["db"])
            va, vb = _grad_views(ga[i], c.dims), _grad_views(base[i], c.dims)
            use = 0.0
            for kind in ("dW", "db"):
                for l in range(c.L):
                    total = (vb[kind][l] + v[kind][l]).double().cpu()  # fp32 sum of the base and the plain call's gradient
                    use = max(use, R.bound_use(va[kind][l], total, R.accumulate_bound(total)))
            fig["acc"].append(use)
        fig["errs"].append(R.grad_errors(got, bw))
        gb, _, lv, _ = R.grad_bounds(O, site, c.Ms[i], seed=i)
        if not rounded:  # fp32 MFMA: the same rule against the fp32 oracle WITHOUT operand rounding (at least 16 fp32 roundings)
            lv32 = R.class_levels([R.grad_errors(R.oracle_run(O, p, rounded=False)[1], bw)])
            lv = {k: max(lv32.get(k, 0.0), 16 * R.U32) for k in lv}
            gb = {k: R.GRAD_FACTOR * v for k, v in lv.items()}
        fig["bounds"].append(gb)
        fig["levels"].append(lv)
    _bwd[key] = fig
    return fig


def _check_classes(fig, tag, classes):
    bad, worst = [], {}
    for i, (errs, gb, lv) in enumerate(zip(fig["errs"], fig["bounds"], fig["levels"])):
        for (cls, l), e in errs.items():
            if cls not in classes:
                continue
            if e >= worst.get(cls, (-1.0,))[0]:
                worst[cls] = (e, gb[cls], lv[cls])
            if not e <= gb[cls]:
                bad.append((i, cls, l, e, gb[cls]))
    for cls, (e, b, lv) in worst.items():
        record_margin(f"{tag} {cls}", e, b, floor=lv, kind="B gradient slices")
    print(f"{tag}: " + ", ".join(f"{cls} {e:.2e} / {b:.2e}" for cls, (e, b, lv) in worst.items()))
    return bad


BWD_CASES = [c for c in CASES if not (c[0] == "lean" and R.regime(c[1], c[2]) == "small" and c[2] not in (33, 300))]
BWD_IDS = ["-".join(str(v) for v in c) for c in BWD_CASES]


@pytest.mark.parametrize("path,site,M,mode", [c for c in BWD_CASES if c[2] % 4 != 0], ids=[i for c, i in zip(BWD_CASES, BWD_IDS) if c[2] % 4 != 0])
def test_input_gradient_chain_per_row(path, site, M, mode, monkeypatch):
    """B1: the few-row chain, the 32-row many-row chain, the 64-row per-block chain and the persistent one, the per-layer
    path; last activation TANH (goal_enc_tanh: out_act_grad_kernel in front); a problem without parameter gradients."""
    fig = _backward_figures(path, site, M, mode, monkeypatch)
    bad = _check_classes(fig, f"{path} {site} {M} {mode}", ("dx/row",))
    assert fig["finite"] and not bad, bad


@pytest.mark.parametrize("path,site,M,mode", BWD_CASES, ids=BWD_IDS)
def test_weight_and_bias_gradients_per_neuron(path, site, M, mode, monkeypatch):
    """B2: the one-launch few-row kernel, the many-row lean kernels (mlp_wgrad_big_kernel + mlp_wgrad_out_kernel), the
    per-layer path; d_x == NULL where rows % 4 == 0; accumulate = 0 and 1 (small path: mlp_wgrad_reduce_kernel; many rows:
    both reduces)."""
    fig = _backward_figures(path, site, M, mode, monkeypatch)
    tag = f"{path} {site} {M} {mode}"
    bad = _check_classes(fig, tag, ("dW/neuron", "db/group16"))
    for i, use in enumerate(fig["acc"]):
        record_margin(f"{tag} p{i}", use, 1.0, kind="B2 accumulate err / bound")
        if not use <= 1.0:
            bad.append((i, "accumulate", use))
    assert fig["finite"] and not bad, bad


def test_batched_preparation_and_reduces_equal_the_plain_calls(monkeypatch):
    """ops.prep_batch (the weight transposes of two sites as one launch) and ops.reduce_batch (their slab reduces as one):
    d_x and every gradient bit for bit those of the plain calls, whose values B1 / B2 check."""
    from tacorl_amd import ops

    calls = [_Call("save", "q_head", 300, "mixed", monkeypatch).forward(), _Call("save", "goal_enc_tanh", 33, "mixed", monkeypatch).forward()]
    res = []
    for batched in (False, True):
        out = []
        if batched:
            with ops.prep_batch():
                for c in calls:
                    ops.mlp_bwd_fused_pack(c.flats, c.Ms, c.dims, c.tag + "_b", c.dev)
        with ops.reduce_batch(auto=batched):
            for c in calls:
                dx = [torch.full((m, c.ld), NAN, device=c.dev) for m in c.Ms]
                gr = [torch.full_like(f, NAN) for f in c.flats]
                ops.mlp_bwd_fused_dgrad(c.flats, c.bufs, c.douts, c.dims[-1], dx, c.ld, c.Ms, c.dims, c.acts, c.tag + "_b", prepacked=batched)
                ops.mlp_bwd_fused_wgrad(c.xs, c.ld, c.bufs, c.douts, c.dims[-1], gr, c.Ms, c.dims, c.acts, c.tag + "_b")
                out.append((dx, gr))
        torch.cuda.synchronize()
        res.append(out)
    bad = []
    for ci, ((dx0, g0), (dx1, g1)) in enumerate(zip(*res)):
        for i in range(len(dx0)):
            K0 = calls[ci].dims[0]
            if not torch.equal(dx0[i][:, :K0], dx1[i][:, :K0]) or not torch.isfinite(dx1[i][:, :K0]).all():
                bad.append((ci, i, "d_x"))
            if not torch.equal(g0[i].view(torch.int32), g1[i].view(torch.int32)):
                bad.append((ci, i, "gradients"))
    assert not bad, bad


# ===================================================================================================== B3
@pytest.mark.parametrize("site,M,lean", [("q_head", 300, False), ("goal_enc_tanh", 300, False), ("q_head", 4224, True), ("q_head", 33024, True)])
def test_gradients_of_a_problem_are_the_sum_of_its_halves(site, M, lean, monkeypatch):
    """300 = 150 + 150 (few rows), 4224 = 2112 + 2112 (32-row many-row kernels), 33024 = 16512 + 16512 (persistent): the halves
    stay in the regime of the whole and pad alike, so every row's dZ is the whole's and the sums differ by order only."""
    h = M // 2
    assert R.regime(site, h, lean) == R.regime(site, M, lean)
    assert R.regime(site, M, lean) == "small" or R.padded(h) * 2 == R.padded(M)  # (the few-row kernels pad nothing)
    whole = _Call("lean" if lean else "save", site, M, "one", monkeypatch).forward()
    _, gw = whole.backward(False)
    halves = _Call("lean" if lean else "save", site, M, "one", monkeypatch)
    halves.Ms, halves.many = [h, h], whole.many * 2
    halves.xs = [whole.xs[0][:h].contiguous(), whole.xs[0][h:].contiguous()]
    halves.douts = [whole.douts[0][:h].contiguous(), whole.douts[0][h:].contiguous()]
    halves.flats, halves.fb, halves.tag = whole.flats * 2, whole.fb * 2, whole.tag + "_h"
    halves.forward()
    _, gh = halves.backward(False)
    terms = R.reference(site, M, saves="lean" if whole.many[0] else "fp32")[3]
    vw, va, vb = _grad_views(gw[0], whole.dims), _grad_views(gh[0], whole.dims), _grad_views(gh[1], whole.dims)
    worst, worst_wc, where = 0.0, 0.0, None
    for kind in ("dW", "db"):
        for l in range(whole.L):
            both = va[kind][l].double().cpu() + vb[kind][l].double().cpu()
            use = R.bound_use(vw[kind][l], both, R.additivity_bound(terms, kind, l, M))
            worst_wc = max(worst_wc, R.bound_use(vw[kind][l], both, R.additivity_bound(terms, kind, l, M, worst_case=True)))
            if use >= worst:
                worst, where = use, f"{kind}{l}"
    print(f"{site} {M} = 2 x {h}: worst element {worst:.3g} x the bound ({worst_wc:.3g} x the worst-case bound) in {where}")
    record_margin(f"{site} {M} {where}", worst, 1.0, kind="B3 additivity err / bound")
    record_margin(f"{site} {M} {where}", worst_wc, 1.0, kind="B3 additivity err / worst-case bound")
    assert worst <= 1.0, (worst, where)


# ===================================================================================================== B4
def test_refusals_come_before_any_launch(monkeypatch):
    """TACORL_EINVAL / TACORL_ENOMEM, and not a byte of the NaN-filled buffers written: last activation SiLU or ReLU in the
    backward, a workspace one byte short, a misaligned params_bf16 (also in the few-row problem of a call whose many-row
    problem would launch first), ldx % 4 != 0, a hidden width that is no multiple of 8, 9 problems, 5 layers."""
    from tacorl_amd import _lib, ops

    lib = _lib.lib()
    c = _Call("lean", "q_head", 2049, "mixed", monkeypatch)
    dev, n, L, NL = c.dev, 2, c.L, c.dims[-1]
    bufs = [torch.full((ops.mlp_act_layout(m, c.dims, c.acts)[2],), NAN, device=dev) for m in c.Ms]
    nb = lib.tacorl_mlp_bwd_fused_ws_bytes(n, ops.int_array(c.Ms), L, ops.int_array(c.dims))
    ws = torch.full((nb // 4 + 1,), NAN, device=dev)
    dx = [torch.full((m, c.ld), NAN, device=dev) for m in c.Ms]
    gr = [torch.full_like(f, NAN) for f in c.flats]
    P, I = ops.ptr_array, ops.int_array

    def fwd(nprob=n, ldx=c.ld, fb=None, dims=c.dims, acts=c.acts, lean=1):
        k = max(nprob, n)
        rep = lambda v: (v * k)[:nprob]  # noqa: E731
        return lib.tacorl_mlp_fwd_fused(nprob, P(rep(c.xs)), ldx, P(rep(c.flats)), P(rep(c.fb)) if fb is None else fb, P(rep(bufs)),
                                        I(rep(c.Ms)), len(dims) - 1, I(dims), I(acts), lean, ops.stream())

    def dgrad(nprob=n, acts=c.acts, dims=c.dims, ws_bytes=nb):
        rep = lambda v: (v * max(nprob, n))[:nprob]  # noqa: E731
        return lib.tacorl_mlp_bwd_fused_dgrad(nprob, P(rep(c.flats)), P(rep(bufs)), P(rep(c.douts)), NL, P(rep(dx)), c.ld, I(rep(c.Ms)),
                                              len(dims) - 1, I(dims), I(acts), 2, ops.ptr(ws), ws_bytes, ops.stream())

    def wgrad(nprob=n, dims=c.dims, acts=c.acts, ws_bytes=nb):
        rep = lambda v: (v * max(nprob, n))[:nprob]  # noqa: E731
        return lib.tacorl_mlp_bwd_fused_wgrad(nprob, P(rep(c.xs)), c.ld, P(rep(bufs)), P(rep(c.douts)), NL, P(rep(gr)), I(rep(c.Ms)),
                                              len(dims) - 1, I(dims), I(acts), 0, 1, ops.ptr(ws), ws_bytes, ops.stream())

    def misaligned(which):
        a = (C.c_void_p * n)(*[t.data_ptr() for t in c.fb])
        a[which] = c.fb[which].data_ptr() + 2
        return a

    five = [72, 256, 256, 256, 256, 1]
    got = {
        "last activation SiLU": (dgrad(acts=[2, 2, 2, 2]), EINVAL),
        "last activation ReLU": (dgrad(acts=[2, 2, 2, 1]), EINVAL),
        "dgrad workspace one byte short": (dgrad(ws_bytes=nb - 1), ENOMEM),
        "wgrad workspace one byte short": (wgrad(ws_bytes=nb - 1), ENOMEM),
        "pack workspace one byte short": (lib.tacorl_mlp_bwd_fused_pack(n, P(c.flats), I(c.Ms), L, I(c.dims), ops.ptr(ws), nb - 1, ops.stream()), ENOMEM),
        "misaligned params_bf16, many-row problem": (fwd(fb=misaligned(0)), EINVAL),
        "misaligned params_bf16, few-row problem": (fwd(fb=misaligned(1)), EINVAL),
        "ldx % 4 != 0": (fwd(ldx=73), EINVAL),
        "hidden width 100": (fwd(dims=[71, 100, 256, 256, 1]), EINVAL),
        "9 problems forward": (fwd(nprob=9), EINVAL),
        "9 problems dgrad": (dgrad(nprob=9), EINVAL),
        "9 problems wgrad": (wgrad(nprob=9), EINVAL),
        "5 layers forward": (fwd(dims=five, acts=[2, 2, 2, 2, 0]), EINVAL),
        "5 layers dgrad": (dgrad(dims=five, acts=[2, 2, 2, 2, 0]), EINVAL),
        "5 layers wgrad": (wgrad(dims=five, acts=[2, 2, 2, 2, 0]), EINVAL),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    untouched = all(bool(torch.isnan(t).all()) for t in bufs + dx + gr + [ws])
    assert not wrong, wrong
    assert untouched
