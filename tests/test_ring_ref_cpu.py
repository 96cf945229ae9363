"""Conditions on the ring GEMM's fp64 reference and on the shape tables of tests/test_ring_fp64_gpu.py - nothing here runs a
kernel.  (1) The tables reach every instantiation of rnn_gemm_kernel, both weight-gradient tile maps and the ring edges
(nk = 1, S - 1, S, S + 1, > 2 S for some ring depth S; an N-tile count that leaves workgroups of the XCD map idle).  (2) A
correct fp32 implementation - plain fp32 torch with the kernel's order of additions - stays inside every bound and leaves
fewer undecidable ReLU gates than the cap.  (3) Each planted fault, applied to the fp64 result of a listed shape, exceeds
its bound by FAULT_RATIO on the elements it touches (exact checks: it breaks the equality), where the whole-tensor norm of
tests/test_kernels_gpu.py (1e-5 of the Frobenius norm over the output) would be the only other witness."""
import pytest
import torch

from tests import ring_ref as R


# ------------------------------------------------------------------------------------------------- (1) coverage
def test_tables_state_the_routes():
    for (M, K, N), want in R.G1.items():
        assert R.route("fwd", 1, M, 0, K, N) == want, (M, K, N)
    assert R.route("bwd_step", 1, *[R.G1_BWD_STEP[0], 0, R.G1_BWD_STEP[1], R.G1_BWD_STEP[2]]) == ("64x32/4", "xcd")
    for (entry, nprob, M, M2, K, N, ext), want in R.G2.items():
        assert R.route(entry, nprob, M, M2, K, N)[0] == want, (entry, nprob, M, M2, K, N)
        assert ext is None or len(ext) == nprob
    for (nprob, M, K, N, ldx, ldy), want in R.G3.items():
        assert R.route("ld", nprob, M, 0, K, N)[0] == want
        assert ldx >= K and ldx % 8 == 0 and ldy >= N and ldy % 4 == 0
    for (M, N), want in R.W1_MN.items():
        assert R.wgrad_map(M, N) == want, (M, N)


def test_every_template_map_and_ring_edge_is_reached():
    reached, edges = set(), {}
    for entry, nprob, M, M2, K, N, nks in R.ring_cases():
        tile, tmap = R.route(entry, nprob, M, M2, K, N)
        reached.add((tile, tmap))
        S = R.TEMPLATES[tile][2]
        for nk in nks:
            for name, hit in (("1", nk == 1), ("S-1", nk == S - 1), ("S", nk == S), ("S+1", nk == S + 1), (">2S", nk > 2 * S)):
                if hit:
                    edges.setdefault(name, set()).add((tile, nk))
    assert {t for t, _ in reached} == set(R.TEMPLATES), reached
    assert ("64x64/3", "plain") in reached and all(m == "xcd" for t, m in reached if t != "64x64/3")
    assert set(edges) == {"1", "S-1", "S", "S+1", ">2S"}, edges
    # below the prologue depth of the 4-stage ring (RB_S - 1 = 3 stages issued ahead): nk = 1 and 2; just past it: 5
    deep = {nk for e, n, M, M2, K, N, nks in R.ring_cases() if R.route(e, n, M, M2, K, N)[0] == "64x32/4" for nk in nks}
    assert {1, 2, 3, 5} <= deep, deep
    # N tiles that are no multiple of 8 under the XCD map: workgroups return early
    idle = {(M, K, N): R.idle_tiles(R.route("fwd", 1, M, 0, K, N)[0], N) for (M, K, N) in R.G1 if R.G1[(M, K, N)][1] == "xcd"}
    assert idle[(70, 128, 96)] == 5 and idle[(100, 640, 288)] == 7 and idle[(3700, 128, 576)] == 7, idle
    assert 4100 % 128 == 4 and 300 % 16 != 0 and 300 // 128 == 2  # the ragged tile; the twin boundary inside a tile and a fragment
    assert set(R.W1_MN.values()) == {"plain", "xcd-block"} and {r // R.WG_RMIN for r in R.W1_R} == {1, 2, 5}
    assert {R.wgrad_map(M, N) for M, N in R.W2_MN} == {"plain", "xcd-block"}
    for (Rr, slabs, rows, Mp, N) in R.W3:
        assert Rr % (R.WG_RMIN * slabs) == 0 and rows <= Mp and Mp % R.WG_T == 0 and N % R.WG_T == 0


# ----------------------------------------------------------------------------------- (2) fp32 stays inside the bounds
FWD = [("fwd",) + k for k in R.G1] + [("bwd_step",) + R.G1_BWD_STEP]


@pytest.mark.parametrize("case", FWD + list(R.G2) + [("ld",) + k for k in R.G3], ids=str)
def test_fp32_torch_stays_inside_the_bound(case):
    if case[0] in ("fwd", "bwd_step"):
        _, M, K, N = case
        probs = [R.problem(M, K, N, seed=M + K + N, bias=case[0] == "fwd", mask=case[0] == "bwd_step")]
    elif case[0] == "ld":
        probs = R.g3_problems(case[1:])
    else:
        probs = R.g2_problems(case)
    worst, ties, total = 0.0, 0, 0
    for p in probs:
        for twin in ([False, True] if p["M2"] else [False]):
            r64, r32 = R.linear(p, twin=twin), R.linear(p, torch.float32, twin=twin)
            for act in (R.ACTS if case[0] != "bwd_step" else [R.ACT_NONE]):
                b, t = R.bound(r64, act)
                worst = max(worst, R.use(R.output(r32, act), R.output(r64, act), b))
                if act == R.ACT_RELU:
                    ties, total = ties + t, total + b.numel()
    print(case, f"fp32 torch uses {worst:.3g} of the bound; undecidable ReLU gates {ties} of {total}")
    assert worst <= 1.0
    assert ties < R.GATE_CAP * max(total, 1)


@pytest.mark.parametrize("M,N", list(R.W1_MN))
def test_fp32_torch_wgrad_stays_inside_the_bound(M, N):
    for Rr in R.W1_R:
        p = R.wgrad_problem(Rr, M, N, seed=Rr + M + N)
        r64, r32 = R.wgrad(p["dz"], p["x"]), R.wgrad(p["dz"], p["x"], torch.float32)
        assert R.use(r32["dW"], r64["dW"], R.wgrad_bound(r64["magW"], Rr)) <= 1.0
        assert R.use(r32["db"], r64["db"], R.wgrad_bound(r64["magb"], Rr)) <= 1.0
        assert float(r64["db"].abs().min()) > 0  # a mean: no bias sum is a pure cancellation


# ------------------------------------------------------------------------------------------------ (3) planted faults
def _ratio(fault, ref, bnd, where):
    """err / bound of the faulty result on the affected elements (`where`: a bool mask); NaN counts as infinite."""
    err = (fault.double() - ref.double()).abs()
    q = err / bnd.clamp_min(1e-300)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return q[where]


def _seen(q, share=0.5):
    """The fault exceeds FAULT_RATIO x the bound on its worst element and on at least `share` of the affected ones."""
    assert q.numel() and float(q.max()) >= R.FAULT_RATIO, float(q.max())
    assert float((q >= R.FAULT_RATIO).double().mean()) >= share, float((q >= R.FAULT_RATIO).double().mean())
    return float(q.median())


def _rows(M, N, *rows):
    m = torch.zeros(M, N, dtype=torch.bool)
    m[list(rows)] = True
    return m


def test_faults_of_the_main_loop_and_the_store():
    M, K, N = 100, 640, 288  # G1
    p = R.problem(M, K, N, seed=5)
    r = R.linear(p)
    ref, (b, _) = R.output(r, R.ACT_NONE), R.bound(r, R.ACT_NONE)
    # one 16-byte K chunk (8 bf16) of one row dropped
    q = dict(p, x=p["x"].clone())
    q["x"][41, 8 * 13: 8 * 14] = 0
    a = _seen(_ratio(R.output(R.linear(q), 0), ref, b, _rows(M, N, 41)))
    # two adjacent output columns of a lane's four swapped (columns 4 g + 1 and 4 g + 2 of every 16-column fragment)
    sw = ref.clone()
    sw[:, 1::16], sw[:, 2::16] = ref[:, 2::16], ref[:, 1::16]
    cols = torch.zeros(M, N, dtype=torch.bool)
    cols[:, 1::16] = cols[:, 2::16] = True
    c = _seen(_ratio(sw, ref, b, cols))
    # the last ragged row served from its clamped neighbour
    cl = ref.clone()
    cl[M - 1] = ref[M - 2]
    d = _seen(_ratio(cl, ref, b, _rows(M, N, M - 1)))
    # the gap the per-element bound closes: ONE element off by 2 % of the RMS output is FAULT_RATIO x over its bound, and
    # 1e-5 of the Frobenius norm of a 2048 x 2048 output of this scale (tests/test_kernels_gpu.py) does not see it
    one = ref.clone()
    rms = float(ref.norm()) / (M * N) ** 0.5
    delta = 0.02 * rms
    one[57, 100] += delta
    assert float(_ratio(one, ref, b, one != ref)) >= R.FAULT_RATIO
    assert delta / (rms * 2048) < 1e-5
    print(f"median err / bound: chunk {a:.3g}, swap {c:.3g}, clamp {d:.3g}")


def test_faults_of_the_epilogue_operands():
    M, K, N, ld_add = 70, 128, 96, 100  # G1, ld_add = N + 4
    p = R.problem(M, K, N, seed=6, bias2=True, mask=True)
    r = R.linear(p)
    ref, (b, _) = R.output(r, R.ACT_RELU), R.bound(r, R.ACT_RELU)
    open_ = r["gate"]
    # bias2 omitted
    _seen(_ratio(R.output(R.linear(dict(p, b2=None)), R.ACT_RELU), ref, b, open_ & (ref > 0)))
    # addend read at pitch N instead of ld_add: rows >= 1 start inside the NaN pad columns or another row
    whole, _ = R.padded(p["ad"], ld_add)
    flat = whole.reshape(-1)[R.GUARD * ld_add:]
    wrong = flat[: M * N].reshape(M, N)
    assert torch.equal(wrong[0], p["ad"][0])
    _seen(_ratio(R.output(R.linear(dict(p, ad=wrong)), R.ACT_RELU), ref, b, _rows(M, N, *range(1, M)) & open_))
    # the mask taken at pitch N instead of ldy (the strided form: ldy = 3 N, the gap columns NaN)
    mwhole, _ = R.padded(p["mask"], 3 * N)
    mwrong = mwhole.reshape(-1)[R.GUARD * 3 * N:][: M * N].reshape(M, N)
    bad = R.output(R.linear(dict(p, mask=mwrong)), R.ACT_RELU)
    changed = (mwrong > 0) != open_
    assert float(changed[1:].double().mean()) > 0.25
    _seen(_ratio(bad, ref, torch.where(open_, b, R.bound(dict(r, gate=None), R.ACT_RELU)[0]), changed & (R.output(dict(r, gate=None), 1) > 0)), share=0.9)
    # +0.0 and -0.0 in the mask source gate to 0
    z0 = p["mask"] == 0
    assert int(z0.sum()) > 100 and bool(torch.signbit(p["mask"][z0]).any()) and not bool(torch.signbit(p["mask"][z0]).all())
    assert float(ref[z0].abs().max()) == 0.0 and float(b[z0].max()) == 0.0


def test_faults_of_the_twin_the_extension_and_the_copy():
    entry, nprob, M, M2, K, N, _ = ("twin", 3, 300, 212, 384, 128, None)  # G2
    p = R.problem(M, K, N, seed=7, M2=M2, ext=40, bias2=True)
    r2 = R.linear(p, twin=True)
    ref2, (b2, _) = R.output(r2, R.ACT_RELU), R.bound(r2, R.ACT_RELU)
    # twin rows reading x instead of x2
    wrong = R.output(R.linear(dict(p, x2=p["x"][:M2], xe2=p["xe"][:M2]), twin=True), R.ACT_RELU)
    _seen(_ratio(wrong, ref2, b2, (ref2 > 0) | (wrong > 0)), share=0.9)
    # twin rows taking the mask (they have none)
    assert R.linear(dict(p, mask=torch.zeros(M, N)), twin=True)["gate"] is None
    # the extension tile skipped when x == NULL
    pn = R.problem(64, 128, 96, seed=8, ext=40, bias2=True, x_null=True)  # G2 ("ext", 1, 64, ...)
    r = R.linear(pn)
    assert r["n"] == R.RB_K + 3
    ref, (b, _) = R.output(r, R.ACT_NONE), R.bound(r, R.ACT_NONE)
    _seen(_ratio(R.output(R.linear(dict(pn, xe=None)), 0), ref, b, torch.ones_like(ref, dtype=torch.bool)), share=0.9)
    # the zero padding of the extension is contract: it contributes nothing
    assert float(pn["xe"][:, 40:].abs().max()) == 0 and float(pn["we"][:, 40:].abs().max()) == 0
    # bf16 copy by truncation: breaks the exact comparison with round-to-nearest-even
    y32 = R.output(R.linear(pn, torch.float32), 0)
    assert float((R.bf16_trunc(y32) != y32.to(torch.bfloat16)).double().mean()) > 0.3


def test_faults_of_the_weight_gradient():
    Rr, M, N = 320, 512, 256  # W1
    p = R.wgrad_problem(Rr, M, N, seed=9)
    r = R.wgrad(p["dz"], p["x"])
    bW, bb = R.wgrad_bound(r["magW"], Rr), R.wgrad_bound(r["magb"], Rr)
    every = torch.ones(M, N, dtype=torch.bool)
    # four reduction rows dropped from dW
    keep = torch.ones(Rr, dtype=torch.bool)
    keep[100:104] = False
    a = _seen(_ratio(R.wgrad(p["dz"][keep], p["x"][keep])["dW"], r["dW"], bW, every), share=0.9)
    # db taken from the wrong M tile
    _seen(_ratio(r["db"].roll(R.WG_T), r["db"], bb, torch.ones(M, dtype=torch.bool)), share=0.9)
    # one slab left out (W3: R 384 in 3 slabs)
    Rr, slabs, rows, Mp, N = R.W3[1]
    p = R.wgrad_problem(Rr, Mp, N, seed=10, rows=rows)
    r = R.wgrad(p["dz"], p["x"])
    part = R.wgrad(p["dz"][: Rr // slabs * (slabs - 1)], p["x"][: Rr // slabs * (slabs - 1)])
    live = torch.zeros(Mp, N, dtype=torch.bool)
    live[:rows] = True
    _seen(_ratio(part["dW"], r["dW"], R.wgrad_bound(r["magW"], Rr), live), share=0.9)
    assert float(r["dW"][rows:].abs().max()) == 0.0  # the zero columns of dz are contract
    print(f"four dropped rows: median err / bound {a:.3g}")
