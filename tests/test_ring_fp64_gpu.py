"""The ring GEMM and its weight gradients (tacorl_amd/csrc/rnn_ops.hip) per element against the fp64 restatement of
tests/ring_ref.py, at the shapes where the kernel changes: every tile template and workgroup map, ring depths around the
prologue, ragged last tiles, N-tile counts that leave workgroups of the XCD map idle, the twin boundary inside a fragment.

  G1  tacorl_rnn_linear_fwd with bias, addend (ld_add = N + 4) and every act; tacorl_rnn_linear_bwd_step with the mask
  G2  tacorl_rnn_linear_fwd_batch, _twin and _ext: optional operands rotating over the problems, y == NULL, x == NULL
  G3  tacorl_rnn_linear_ld: column slices of shared buffers, the gaps and the other slices still NaN; refusals
  G4  one row, one bit pattern: a probe row's output bits do not depend on the entry, the tile template, the ring depth, the
      map, the row's place, the problem's place, the twin, NULL-operand or strided form
  W1  tacorl_rnn_wgrad on both tile maps, accumulate 0 / 1, db present / NULL
  W2  tacorl_rnn_wgrad_batch: bit-identical to single launches
  W3  tacorl_rnn_wgrad_slabs: the fp32 sum of the slabs' single launches in slab order, bit for bit; ENOMEM before any write

Bounds: |got - ref| <= 2 n 2^-24 (sum |x||w| + |b| + |b2| + |addend|) with n the number of terms (ring_ref.bound,
ring_ref.wgrad_bound); SiLU / Tanh add 4 x plain fp32 torch's error on the same z; the bf16 copy is bf16(y) exactly.  Every
input lies inside NaN (pad columns, guard rows), every output is NaN-prefilled with guard rows.  tests/test_ring_ref_cpu.py
shows what the bounds still detect.  A test collects all its figures before it asserts and records the worst err / bound per
(entry, route) through golden_util.record_margin (tools/ring_margins_md.py -> profiles/ring_margins.md)."""
import ctypes as C

import pytest
import torch

from tests import ring_ref as R
from tests.golden_util import record_margin
from tests.test_action_decoder_gpu import _guarded, _untouched

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -22, -12
NAN = float("nan")
OUT_GUARD = 3  # _guarded's guard rows


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _put(t, dev, ld=None, col=0):
    """An input on the device inside NaN pad columns and guard rows (1-D: as it is), as the column slice that starts at `col`;
    the view the kernel is given."""
    if t is None:
        return None
    if t.dim() == 1:
        return t.to(dev)
    whole, _ = R.padded(t, ld, col=col)
    return whole.to(dev)[R.GUARD: R.GUARD + t.shape[0], col:]


class _Figures:
    """Worst err / bound and undecidable gates per (entry, tile, map, class), with the shape that produced the worst.  Class
    "sum": outputs whose bound is the accumulation's alone (act none / ReLU, weight gradients); "act": SiLU / Tanh outputs,
    whose bound adds the activation's tolerance."""

    def __init__(self):
        self.rows, self.bad = {}, []

    def add(self, entry, route, shape, use, ties=0, note="", cls="sum"):
        k = (entry,) + tuple(route) + (cls,)
        old = self.rows.get(k, (-1.0, 0, ""))
        self.rows[k] = (max(old[0], use), old[1] + ties, shape if use > old[0] else old[2])
        if not use <= 1.0:
            self.bad.append(f"{entry} {route} {shape} {note}: err / bound {use:.3g}")

    def finish(self):
        for (entry, tile, tmap, cls), (use, ties, shape) in self.rows.items():
            print(f"ring err / bound {entry} {tile} {tmap} {cls}: {use:.3g} ({ties} undecidable gates) at {shape}")
            record_margin(f"{entry}|{tile}|{tmap}|{cls}|{shape}", use, 1.0, floor=ties, kind="ring err / bound")
        assert not self.bad, "\n".join(self.bad)


def _verify(fig, entry, route, shape, p, act, y, yb, twin=False, ref=None):
    """One problem's outputs (fp32 y and / or its bf16 copy, CPU tensors) against fp64; gates counted against the cap."""
    r = ref or R.linear(p, twin=twin)
    want = R.output(r, act)
    b, ties = R.bound(r, act)
    if ties >= R.GATE_CAP * b.numel():
        fig.bad.append(f"{entry} {shape}: {ties} undecidable gates of {b.numel()}")
    note, cls = ("twin " if twin else "") + f"act {act}", "act" if act in (R.ACT_SILU, R.ACT_TANH) else "sum"
    if y is not None:
        fig.add(entry, route, shape, R.use(y, want, b), ties, note, cls)
        if yb is not None and not torch.equal(_bits(yb), _bits(y.to(torch.bfloat16))):
            fig.bad.append(f"{entry} {route} {shape} {note}: the bf16 copy is not bf16(y)")
    else:
        fig.add(entry, route, shape, R.use(yb.float(), want, R.copy_bound(want, b)), ties, note + " copy only", cls)


# ======================================================================================================== G1
@pytest.mark.parametrize("M,K,N", list(R.G1))
def test_g1_linear_fwd(M, K, N):
    """tacorl_rnn_linear_fwd, every act on one problem (bias, addend at ld_add = N + 4)."""
    from tacorl_amd import _lib, ops

    dev, fig, route = _dev(), _Figures(), R.route("fwd", 1, M, 0, K, N)
    assert route == R.G1[(M, K, N)]
    p = R.problem(M, K, N, seed=M + K + N)
    x, w, b, ad = _put(p["x"], dev), _put(p["w"], dev), _put(p["b"], dev), _put(p["ad"], dev, N + 4)
    r = R.linear(p)
    for act in R.ACTS:
        (y, y_all), (yb, yb_all) = _guarded(M, N, dev), _guarded(M, N, dev, torch.bfloat16)
        rc = _lib.lib().tacorl_rnn_linear_fwd(ops.ptr(x), ops.ptr(w), ops.ptr(b), ops.ptr(ad), N + 4, ops.ptr(y), ops.ptr(yb), M, K, N,
                                              act, ops.stream())
        torch.cuda.synchronize()
        assert rc == 0
        _verify(fig, "fwd", route, (M, K, N), p, act, y.cpu(), yb.cpu(), ref=r)
        _untouched(f"fwd {M, K, N} act {act}", y_all, M)
        _untouched(f"fwd {M, K, N} act {act} bf16", yb_all, M)
    fig.finish()


def test_g1_bwd_step():
    """tacorl_rnn_linear_bwd_step: y = (x Wt^T + addend) [mask_src > 0]; +0.0 and -0.0 of the mask source gate to 0."""
    from tacorl_amd import _lib, ops

    M, K, N = R.G1_BWD_STEP
    dev, fig, route = _dev(), _Figures(), R.route("bwd_step", 1, M, 0, K, N)
    p = R.problem(M, K, N, seed=M + K + N, bias=False, mask=True)
    (y, y_all), (yb, yb_all) = _guarded(M, N, dev), _guarded(M, N, dev, torch.bfloat16)
    x, w, ad, ms = _put(p["x"], dev), _put(p["w"], dev), _put(p["ad"], dev, N + 4), _put(p["mask"], dev)
    rc = _lib.lib().tacorl_rnn_linear_bwd_step(ops.ptr(x), ops.ptr(w), ops.ptr(ad), N + 4, ops.ptr(ms), ops.ptr(y), ops.ptr(yb), M, K, N,
                                               ops.stream())
    torch.cuda.synchronize()
    assert rc == 0
    _verify(fig, "bwd_step", route, (M, K, N), p, R.ACT_NONE, y.cpu(), yb.cpu())
    assert not bool(y.cpu()[p["mask"] == 0].any())
    _untouched("bwd_step", y_all, M)
    _untouched("bwd_step bf16", yb_all, M)
    fig.finish()


# ======================================================================================================== G2
def _batch_launch(entry, D, M, M2, K, N, ld_add):
    from tacorl_amd import _lib, ops

    pa, lib, n = ops.ptr_array, _lib.lib(), len(D)
    g = lambda k: pa([d.get(k) for d in D])  # noqa: E731
    acts = ops.int_array([d["act"] for d in D])
    if entry == "fwd_batch":
        rc = lib.tacorl_rnn_linear_fwd_batch(n, g("x"), g("w"), g("b"), g("ad"), ld_add, g("y"), g("yb"), M, K, N, acts, ops.stream())
    elif entry == "twin":
        rc = lib.tacorl_rnn_linear_fwd_batch_twin(n, g("x"), g("x2"), g("w"), g("b"), g("ad"), g("ad2"), ld_add, g("y"), g("y2"), g("yb"),
                                                  g("yb2"), M, M2, K, N, acts, ops.stream())
    elif entry == "ext":
        tw = (lambda k: g(k)) if M2 else (lambda k: None)  # noqa: E731
        rc = lib.tacorl_rnn_linear_fwd_batch_ext(n, g("x"), tw("x2"), g("w"), g("b"), g("ad"), tw("ad2"), ld_add, g("y"), tw("y2"), g("yb"),
                                                 tw("yb2"), M, M2, K, N, acts, g("xe"), tw("xe2"), g("we"), g("b2"), ops.stream())
    else:
        assert entry == "bwd_batch"
        rc = lib.tacorl_rnn_linear_bwd_batch(n, g("x"), g("w"), g("ad"), ld_add, g("mask"), g("y"), g("yb"), M, K, N, ops.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("key", list(R.G2), ids=lambda k: f"{k[0]}-n{k[1]}-M{k[2]}+{k[3]}-K{k[4]}-N{k[5]}" + ("-ext" if k[6] else ""))
def test_g2_linear_fwd_batch(key):
    """The batched entries.  Problem p: addend unless p % 3 == 1, bf16 copy unless p % 3 == 1, y == NULL (the copy alone)
    where p % 3 == 2; the K extension and x == NULL as R.G2 lists them; twin rows carry no mask and their own buffers."""
    entry, nprob, M, M2, K, N, ext = key
    dev, fig = _dev(), _Figures()
    route = R.route(entry, nprob, M, M2, K, N)
    assert route[0] == R.G2[key]
    P, ld_add = R.g2_problems(key), N + 4
    D, outs = [], []
    for i, p in enumerate(P):
        d = {k: _put(p.get(k), dev) for k in ("x", "w", "b", "b2", "xe", "we", "x2", "xe2")}
        d["ad"], d["ad2"], d["act"] = _put(p.get("ad"), dev, ld_add), _put(p.get("ad2"), dev, ld_add), p["act"]
        o = dict(y=_guarded(M, N, dev) if i % 3 != 2 else (None, None),
                 yb=_guarded(M, N, dev, torch.bfloat16) if i % 3 != 1 else (None, None))
        if M2:
            o["y2"] = _guarded(M2, N, dev)
            o["yb2"] = _guarded(M2, N, dev, torch.bfloat16) if i % 3 != 1 else (None, None)
        d.update({k: v[0] for k, v in o.items()})
        D.append(d)
        outs.append(o)
    assert _batch_launch(entry, D, M, M2, K, N, ld_add) == 0
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    for i, (p, o) in enumerate(zip(P, outs)):
        shape = (nprob, M, M2, K, N) + ((ext[i],) if ext else ())
        _verify(fig, entry, route, shape, p, p["act"], cpu(o["y"][0]), cpu(o["yb"][0]))
        if M2:
            _verify(fig, entry, route, shape, p, p["act"], cpu(o["y2"][0]), cpu(o["yb2"][0]), twin=True)
        for k, (view, whole) in o.items():
            if whole is not None:
                _untouched(f"{entry} {shape} problem {i} {k}", whole, M2 if k.endswith("2") else M)
    fig.finish()


# ======================================================================================================== G3
def _ld_launch(D, ldx, ld_add, ldy, M, K, N, act, nprob=None):
    from tacorl_amd import _lib, ops

    pa = ops.ptr_array
    g = lambda k: pa([d.get(k) for d in D])  # noqa: E731
    rc = _lib.lib().tacorl_rnn_linear_ld(len(D) if nprob is None else nprob, g("x"), ldx, g("w"), g("b"), g("b2"), g("ad"), ld_add, g("xe"),
                                        g("we"), g("mask"), g("y"), g("yb"), ldy, M, K, N, act, ops.stream())
    torch.cuda.synchronize()
    return rc


def _ld_case(key, dev):
    """Problems of a G3 launch on the device.  x: column slices of one [M][ldx] buffer where ldx == 2 K, else one buffer per
    problem with NaN beyond K; the mask sources and the outputs: column slices p N .. (p + 1) N of one [M][ldy] buffer each."""
    nprob, M, K, N, ldx, ldy = key
    P = R.g3_problems(key)
    if ldx == nprob * K:
        xs = _put(torch.cat([p["x"] for p in P], 1), dev)
        xv = [xs[:, i * K:] for i in range(nprob)]
    else:
        xv = [_put(p["x"], dev, ldx) for p in P]
    mask = torch.full((M, ldy), NAN)
    for i, p in enumerate(P):
        mask[:, i * N: (i + 1) * N] = p["mask"]
    mask = _put(mask, dev)
    D = []
    for i, p in enumerate(P):
        d = {k: _put(p.get(k), dev) for k in ("w", "b", "b2", "xe", "we")}
        d.update(x=xv[i], ad=_put(p.get("ad"), dev, N + 4), mask=mask[:, i * N:])
        D.append(d)
    return P, D


def _ld_outputs(D, M, N, ldy, dev):
    y, y_all = _guarded(M, ldy, dev)
    yb, yb_all = _guarded(M, ldy, dev, torch.bfloat16)
    for i, d in enumerate(D):
        d["y"], d["yb"] = y[:, i * N:], yb[:, i * N:]
    return y_all, yb_all


def _only_slices_written(name, whole, M, N, nprob):
    w = whole.float().cpu()
    body = w[OUT_GUARD: OUT_GUARD + M]
    assert torch.isnan(w[:OUT_GUARD]).all() and torch.isnan(w[OUT_GUARD + M:]).all(), f"{name}: written outside its rows"
    assert torch.isnan(body[:, nprob * N:]).all(), f"{name}: written into another column slice"
    return [body[:, i * N: (i + 1) * N] for i in range(nprob)]


@pytest.mark.parametrize("key", list(R.G3), ids=lambda k: f"n{k[0]}-M{k[1]}-K{k[2]}-N{k[3]}-ldx{k[4]}-ldy{k[5]}")
def test_g3_linear_ld(key):
    """tacorl_rnn_linear_ld at act ReLU (a forward step) and none (a BPTT step): strided x, y, bf16 copy and mask source."""
    nprob, M, K, N, ldx, ldy = key
    dev, fig = _dev(), _Figures()
    route = R.route("ld", nprob, M, 0, K, N)
    assert route[0] == R.G3[key]
    P, D = _ld_case(key, dev)
    refs = [R.linear(p) for p in P]
    for act in (R.ACT_RELU, R.ACT_NONE):
        y_all, yb_all = _ld_outputs(D, M, N, ldy, dev)
        assert _ld_launch(D, ldx, N + 4, ldy, M, K, N, act) == 0
        ys, ybs = _only_slices_written("ld y", y_all, M, N, nprob), _only_slices_written("ld y_bf16", yb_all, M, N, nprob)
        for i, p in enumerate(P):
            _verify(fig, "ld", route, key + (i,), p, act, ys[i], ybs[i].to(torch.bfloat16), ref=refs[i])
    fig.finish()


def test_g3_linear_ld_refuses():
    """Refused arguments leave everything NaN: ldx < K, ldx % 8, ldy % 4, an x_ext without its w_ext, a slice 4 bytes off its
    alignment, nprob 0 and 5.  The same call with nothing wrong is taken."""
    key = list(R.G3)[0]
    nprob, M, K, N, ldx, ldy = key
    dev = _dev()
    P, D = _ld_case(key, dev)
    y_all, yb_all = _ld_outputs(D, M, N, ldy, dev)
    go = lambda D_=D, **kw: _ld_launch(D_, kw.pop("ldx", ldx), N + 4, kw.pop("ldy", ldy), M, K, N, R.ACT_RELU, **kw)  # noqa: E731
    off = lambda k: [dict(D[0], **{k: C.c_void_p(D[0][k].data_ptr() + 4)}), D[1]]  # noqa: E731
    five = D + D + D[:1]
    rcs = dict(ldx_small=go(ldx=K - 8), ldx_mod8=go(ldx=ldx + 4), ldy_mod4=go(ldy=ldy + 2), lone_ext=go([dict(D[0], we=None), D[1]]),
               x_off=go(off("x")), y_off=go(off("y")), mask_off=go(off("mask")), nprob0=go(five, nprob=0), nprob5=go(five, nprob=5))
    assert all(rc == EINVAL for rc in rcs.values()), rcs
    assert torch.isnan(y_all).all() and torch.isnan(yb_all.float()).all()
    assert go() == 0
    _only_slices_written("ld y", y_all, M, N, nprob)
    assert torch.isfinite(y_all[OUT_GUARD: OUT_GUARD + M, : nprob * N]).all()


# ======================================================================================================== G4
G4_K, G4_N = 384, 384
# (entry, nprob, M, M2) at K = N = 384 -> the route the launch is here for
G4 = {("fwd", 1, 70, 0): ("64x32/4", "xcd"), ("fwd", 1, 1100, 0): ("64x64/3", "plain"), ("fwd", 1, 5500, 0): ("128x64/3", "xcd"),
      ("bwd_step", 1, 70, 0): ("64x32/4", "xcd"), ("fwd_batch", 1, 64, 0): ("64x32/4", "xcd"), ("fwd_batch", 2, 448, 0): ("64x32/2", "xcd"),
      ("fwd_batch", 4, 200, 0): ("64x32/2", "xcd"), ("fwd_batch", 3, 128, 0): ("128x64/2", "xcd"), ("twin", 3, 300, 212): ("128x128/2", "xcd"),
      ("twin", 1, 40, 24): ("64x32/4", "xcd"), ("ld", 2, 24, 0): ("64x32/4", "xcd"), ("ld", 2, 5500, 0): ("128x64/3", "xcd"),
      ("bwd_batch", 3, 128, 0): ("128x64/2", "xcd"), ("bwd_batch", 2, 64, 0): ("64x32/4", "xcd")}


def _g4_run(dev, probe_x, probe_ad, w, null_x=False, only=None):
    """Every launch of G4 with the probe at rows 0, 15, 16, 63, 64 and the last row (twin rows: 0, 4 - the fragment the twin
    boundary cuts - and the last) of the first and the last problem; the other rows random.  -> [(where, y row, yb row)]."""
    from tacorl_amd import _lib, ops

    K, N, ld_add, lib = G4_K, G4_N, G4_N + 4, _lib.lib()
    wd, got = _put(w, dev), []
    for (entry, nprob, M, M2), want in G4.items():
        if only is not None and (entry, nprob, M, M2) not in only:
            continue
        assert R.route(entry, nprob, M, M2, K, N) == want, (entry, nprob, M, M2)
        g = torch.Generator().manual_seed(M + 7 * nprob)
        at = sorted({r for r in (0, 15, 16, 63, 64, M - 1) if r < M})
        at2 = sorted({r for r in (0, 4, M2 - 1) if r < M2})
        strided = entry == "ld"
        ldx, ldy = (2 * K if M < 64 else K + 8, 3 * N if M < 64 else 2 * N) if strided else (K, N)
        D, outs = [], []
        for i in range(nprob):
            x, ad = R.bf(torch.randn(M, K, generator=g)), torch.randn(M, N, generator=g)
            if i in (0, nprob - 1):
                x[at], ad[at] = probe_x, probe_ad
            d = dict(x=None if null_x else _put(x, dev, ldx if strided and ldx != 2 * K else None), w=wd, ad=_put(ad, dev, ld_add), act=R.ACT_NONE)
            if strided and ldx == 2 * K:  # a column slice of a buffer twice as wide
                d["x"] = _put(torch.cat([x, x], 1), dev)[:, K:]
            o = dict(y=_guarded(M, ldy, dev), yb=_guarded(M, ldy, dev, torch.bfloat16))
            if M2:
                x2, ad2 = R.bf(torch.randn(M2, K, generator=g)), torch.randn(M2, N, generator=g)
                if i in (0, nprob - 1):
                    x2[at2], ad2[at2] = probe_x, probe_ad
                d.update(x2=_put(x2, dev), ad2=_put(ad2, dev, ld_add))
                o.update(y2=_guarded(M2, N, dev), yb2=_guarded(M2, N, dev, torch.bfloat16))
            d.update({k: v[0] for k, v in o.items()})
            D.append(d)
            outs.append(o)
        d = D[0]
        if entry == "fwd":
            rc = lib.tacorl_rnn_linear_fwd(ops.ptr(d["x"]), ops.ptr(wd), None, ops.ptr(d["ad"]), ld_add, ops.ptr(d["y"]), ops.ptr(d["yb"]), M, K, N,
                                           R.ACT_NONE, ops.stream())
        elif entry == "bwd_step":
            rc = lib.tacorl_rnn_linear_bwd_step(ops.ptr(d["x"]), ops.ptr(wd), ops.ptr(d["ad"]), ld_add, None, ops.ptr(d["y"]), ops.ptr(d["yb"]),
                                                M, K, N, ops.stream())
        elif strided:
            rc = _ld_launch(D, ldx, ld_add, ldy, M, K, N, R.ACT_NONE)
        else:
            rc = _batch_launch(entry, D, M, M2, K, N, ld_add)
        torch.cuda.synchronize()
        assert rc == 0, (entry, nprob, M, M2, rc)
        for i in sorted({0, nprob - 1}):
            y, yb = outs[i]["y"][0].cpu()[:, :N], outs[i]["yb"][0].cpu()[:, :N]
            got += [((entry, nprob, M, M2, i, r), y[r], yb[r]) for r in at]
            if M2:
                y2, yb2 = outs[i]["y2"][0].cpu(), outs[i]["yb2"][0].cpu()
                got += [((entry, nprob, M, M2, i, f"twin {r}"), y2[r], yb2[r]) for r in at2]
    return got


def test_g4_one_row_one_bit_pattern():
    """The callers rely on it (test_rnn_linear_fwd_batch_twin across 128 x 128 and 128 x 64 tiles; the NULL operand; the
    module's routes against each other): an output element's bits depend on its own row of x, its addend and its own row of W
    only.  Every template multiplies the same 32-column MFMA steps in the same order (rnn_gemm_kernel: `c = 4 * ks + g` inside
    K tile kt, kt ascending) into an accumulator that starts at +0, and the epilogue is the same code: no route orders the sum
    differently, so every pair is held to bit equality."""
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    probe_x, probe_ad = R.bf(torch.randn(G4_K, generator=g)), torch.randn(G4_N, generator=g)
    w = R.bf(torch.randn(G4_N, G4_K, generator=g) / G4_K ** 0.5)
    got = _g4_run(dev, probe_x, probe_ad, w)
    assert {k[0] for k, _, _ in got} == {"fwd", "bwd_step", "fwd_batch", "twin", "ld", "bwd_batch"} and len(got) > 60
    (k0, y0, yb0), differ = got[0], []
    for k, y, yb in got[1:]:
        if not torch.equal(_bits(y), _bits(y0)) or not torch.equal(_bits(yb), _bits(yb0)):
            differ.append((k, int((_bits(y) != _bits(y0)).sum()), int((_bits(yb) != _bits(yb0)).sum())))
    # the pattern itself against fp64, at the G1 bound
    p = dict(M=1, M2=0, x=probe_x[None], w=w, ad=probe_ad[None])
    r = R.linear(p)
    u = R.use(y0[None], R.output(r, R.ACT_NONE), R.bound(r, R.ACT_NONE)[0])
    record_margin(f"probe row|all routes|-|sum|{(G4_K, G4_N)}", u, 1.0, floor=len(differ), kind="ring err / bound")
    print(f"G4: {len(got)} placements, {len(differ)} differ from {k0}; probe row err / bound {u:.3g}")
    assert torch.equal(_bits(yb0), _bits(y0.to(torch.bfloat16)))
    assert not differ, differ
    assert u <= 1.0


def test_g4_null_operand_row():
    """The same with x == NULL in every problem of the batched launches against a zero row in a buffer (tacorl_rnn_linear_fwd,
    tacorl_rnn_linear_ld): the bits of +0 + addend."""
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    probe_ad = torch.randn(G4_N, generator=g)
    w = R.bf(torch.randn(G4_N, G4_K, generator=g) / G4_K ** 0.5)
    zero = torch.zeros(G4_K, dtype=torch.bfloat16)
    buf = _g4_run(dev, zero, probe_ad, w, only=[("fwd", 1, 70, 0), ("ld", 2, 24, 0), ("fwd_batch", 3, 128, 0)])
    nul = _g4_run(dev, zero, probe_ad, w, null_x=True, only=[k for k in G4 if k[0] == "fwd_batch"])
    assert len(buf) >= 12 and len(nul) >= 16
    want = torch.zeros(G4_N) + probe_ad
    differ = [k for k, y, yb in buf + nul if not torch.equal(_bits(y), _bits(want)) or not torch.equal(_bits(yb), _bits(want.to(torch.bfloat16)))]
    assert not differ, differ


# ======================================================================================================== W1 - W3
def LD(cols):
    """Row pitch of a weight-gradient operand: its columns [8, 8 + cols) of a buffer 24 columns wider, NaN on both sides."""
    return cols + 24


def _vec(n, dev, fill=NAN, guard=4):
    whole = torch.full((n + 2 * guard,), fill, device=dev)
    return whole[guard: guard + n], whole


def _wgrad_single(dz, ld_dz, x, ld_x, Rr, M, N, dw, db, accumulate):
    from tacorl_amd import _lib, ops

    rc = _lib.lib().tacorl_rnn_wgrad(ops.ptr(dz), ld_dz, ops.ptr(x), ld_x, Rr, M, N, ops.ptr(dw), ops.ptr(db), accumulate, ops.stream())
    torch.cuda.synchronize()
    return rc


def _wgrad_check(fig, entry, shape, r, Rr, dw, db, base_w=None, base_b=None):
    tmap = (R.wgrad_map(shape[1], shape[2]), "dW")
    bW, bb = R.wgrad_bound(r["magW"], Rr), R.wgrad_bound(r["magb"], Rr)
    refW, refb = r["dW"], r["db"]
    if base_w is not None:
        refW, refb = refW + base_w.double(), refb + base_b.double()
        bW, bb = R.accumulate_bound(bW, refW), R.accumulate_bound(bb, refb)
    fig.add(entry, tmap, shape, R.use(dw, refW, bW), note="dW" + (" accumulate" if base_w is not None else ""))
    if db is not None:
        fig.add(entry, (tmap[0], "db"), shape, R.use(db, refb, bb), note="db")


@pytest.mark.parametrize("M,N", list(R.W1_MN))
@pytest.mark.parametrize("Rr", R.W1_R)
def test_w1_wgrad(Rr, M, N):
    """tacorl_rnn_wgrad: operands as column slices (columns 8 .. of a buffer 24 columns wider, NaN on both sides), accumulate 0 / 1, db present /
    NULL; dW per element and db over every M tile against fp64; the accumulating call is base + the plain call's result in one
    fp32 addition, bit for bit (`v += *o`)."""
    dev, fig = _dev(), _Figures()
    assert R.wgrad_map(M, N) == R.W1_MN[(M, N)]
    p = R.wgrad_problem(Rr, M, N, seed=Rr + M + N)
    r = R.wgrad(p["dz"], p["x"])
    dz, x = _put(p["dz"], dev, LD(M), 8), _put(p["x"], dev, LD(N), 8)
    bw_, bb_ = R.base((M, N), 1), R.base((M,), 2)
    plain, shape = None, (Rr, M, N)
    for with_db in (True, False):
        for accumulate in (0, 1):
            dw, dw_all = _guarded(M, N, dev)
            db, db_all = _vec(M, dev)
            if accumulate:
                dw.copy_(bw_)
                db.copy_(bb_)
            assert _wgrad_single(dz, LD(M), x, LD(N), Rr, M, N, dw, db if with_db else None, accumulate) == 0
            _untouched(f"wgrad {shape} dW", dw_all, M)
            assert torch.isnan(db_all[:4]).all() and torch.isnan(db_all[4 + M:]).all()
            got_w, got_b = dw.cpu(), db.cpu()
            if not with_db:
                assert torch.equal(_bits(got_b), _bits(bb_)) if accumulate else bool(torch.isnan(got_b).all()), "db == NULL writes nothing"
            _wgrad_check(fig, "wgrad", shape, r, Rr, got_w, got_b if with_db else None, *((bw_, bb_) if accumulate else ()))
            if plain is None:
                plain = (got_w, got_b)
            elif accumulate:
                assert torch.equal(_bits(got_w), _bits(bw_ + plain[0])), "accumulate: base + the plain result"
                assert not with_db or torch.equal(_bits(got_b), _bits(bb_ + plain[1]))
            else:
                assert torch.equal(_bits(got_w), _bits(plain[0])), "dW must not depend on db"
    fig.finish()


@pytest.mark.parametrize("M,N", R.W2_MN)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_w2_wgrad_batch(n, M, N):
    """tacorl_rnn_wgrad_batch: n problems of row counts (64, 192, 128, 320), db present for the even ones; bit-identical to
    single launches, and within the bound against fp64."""
    from tacorl_amd import _lib, ops

    dev, fig = _dev(), _Figures()
    Rs = R.W2_R[:n]
    P = [R.wgrad_problem(Rr, M, N, seed=Rr + M + N + i) for i, Rr in enumerate(Rs)]
    dz, x = [_put(p["dz"], dev, LD(M), 8) for p in P], [_put(p["x"], dev, LD(N), 8) for p in P]
    dws, dbs = [_guarded(M, N, dev) for _ in P], [_vec(M, dev) if i % 2 == 0 else (None, None) for i in range(n)]
    rc = _lib.lib().tacorl_rnn_wgrad_batch(n, ops.ptr_array(dz), LD(M), ops.ptr_array(x), LD(N), ops.int_array(Rs), M, N,
                                           ops.ptr_array([d[0] for d in dws]), ops.ptr_array([d[0] for d in dbs]), 0, ops.stream())
    torch.cuda.synchronize()
    assert rc == 0
    same = []
    for i, p in enumerate(P):
        dw1, dw1_all = _guarded(M, N, dev)
        db1, _ = _vec(M, dev)
        assert _wgrad_single(dz[i], LD(M), x[i], LD(N), Rs[i], M, N, dw1, db1, 0) == 0
        _untouched(f"wgrad_batch problem {i}", dws[i][1], M)
        same.append(torch.equal(_bits(dws[i][0].cpu()), _bits(dw1.cpu())) and (dbs[i][0] is None or torch.equal(_bits(dbs[i][0].cpu()), _bits(db1.cpu()))))
        _wgrad_check(fig, "wgrad_batch", (Rs[i], M, N), R.wgrad(p["dz"], p["x"]), Rs[i], dws[i][0].cpu(), None if dbs[i][0] is None else dbs[i][0].cpu())
    assert all(same), same
    fig.finish()


@pytest.mark.parametrize("Rr,slabs,rows,Mp,N", R.W3)
def test_w3_wgrad_slabs(Rr, slabs, rows, Mp, N):
    """tacorl_rnn_wgrad_slabs: rows < Mp output rows (dz columns [rows, Mp) zero, NaN beyond Mp), R cut into slabs.  The result is
    the fp32 sum, in slab order from +0 (accumulate: from the destination), of tacorl_rnn_wgrad over each row range, bit for bit;
    slabs == 1 is tacorl_rnn_wgrad itself; destination rows >= rows stay untouched; a workspace one byte short is ENOMEM before
    any write."""
    from tacorl_amd import _lib, ops

    dev, fig, lib = _dev(), _Figures(), _lib.lib()
    p = R.wgrad_problem(Rr, Mp, N, seed=Rr + Mp + N, rows=rows)
    r = R.wgrad(p["dz"], p["x"])
    ld_dz, ld_x, Rs = LD(Mp), LD(N), Rr // slabs
    dz, x = _put(p["dz"], dev, ld_dz, 8), _put(p["x"], dev, ld_x, 8)
    need = lib.tacorl_rnn_wgrad_slabs_ws_bytes(slabs, Mp, N)
    assert need == slabs * Mp * (N + 1) * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    bw_, bb_ = R.base((rows, N), 3), R.base((rows,), 4)
    parts = []
    for s in range(slabs):  # the single launches over each row range
        dw1, _ = _guarded(Mp, N, dev)
        db1, _ = _vec(Mp, dev)
        assert _wgrad_single(dz[s * Rs:], ld_dz, x[s * Rs:], ld_x, Rs, Mp, N, dw1, db1, 0) == 0
        parts.append((dw1[:rows].clone(), db1[:rows].clone()))
    for accumulate in (0, 1):
        dw, dw_all = _guarded(rows, N, dev)
        db, db_all = _vec(rows, dev)
        if accumulate:
            dw.copy_(bw_)
            db.copy_(bb_)
        args = (ops.ptr(dz), ld_dz, ops.ptr(x), ld_x, Rr, Mp, N, rows, slabs, ops.ptr(dw), ops.ptr(db), accumulate, ops.ptr(ws))
        if not accumulate:
            assert lib.tacorl_rnn_wgrad_slabs(*args, need - 1, ops.stream()) == ENOMEM
            torch.cuda.synchronize()
            assert torch.isnan(dw_all).all() and torch.isnan(db_all).all() and bool((ws == 0xFF).all()), "ENOMEM comes before any write"
        assert lib.tacorl_rnn_wgrad_slabs(*args, need, ops.stream()) == 0
        torch.cuda.synchronize()
        _untouched(f"wgrad_slabs {Rr, slabs, rows, Mp, N} dW", dw_all, rows)
        assert torch.isnan(db_all[:4]).all() and torch.isnan(db_all[4 + rows:]).all()
        sw = bw_.to(dev) if accumulate else torch.zeros(rows, N, device=dev)
        sb = bb_.to(dev) if accumulate else torch.zeros(rows, device=dev)
        for pw, pb in parts:
            sw, sb = sw + pw, sb + pb
        assert torch.equal(_bits(dw), _bits(sw)), "dW: the fp32 sum of the slabs' single launches in slab order"
        assert torch.equal(_bits(db), _bits(sb)), "db likewise"
        if slabs == 1 and not accumulate:
            assert torch.equal(_bits(dw), _bits(parts[0][0])) and torch.equal(_bits(db), _bits(parts[0][1])), "slabs == 1: tacorl_rnn_wgrad"
        rr = dict(dW=r["dW"][:rows], db=r["db"][:rows], magW=r["magW"][:rows], magb=r["magb"][:rows])
        _wgrad_check(fig, "wgrad_slabs", (Rr, Mp, N), rr, Rr, dw.cpu(), db.cpu(), *((bw_, bb_) if accumulate else ()))
    fig.finish()
