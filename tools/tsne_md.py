"""Write profiles/tsne.md: the bound use of every GPU case of tests/test_tsne_gpu.py, the fp32-restatement deviations its
trajectory tests scaled their tolerance from, and the time of tsne_embed against the same definition written in torch ops.

    python tools/tsne_md.py [--out profiles/tsne.md] [--sizes 1024 4096 8192] [--nbr-sizes 8192 32768 131072] [--no-tests]

Needs a GPU (there is no host path to time).  Times are HIP events around the work on one stream, after one warm-up run of the
same shape, the median of 5.  The torch-op statement is the baseline, not the code under test: the usual dense formulation
(|y_i|^2 + |y_j|^2 - 2 y_i.y_j through a GEMM, row sums and two (N, N) x (N, 2) products for the forces; the perplexity search
vectorised over the rows, every row bisected until all have converged, checked every 10 steps).

A second section times the neighbour-sparse path (tsne_embed_neighbours' launches) at --nbr-sizes, against the dense path at
N = 8192: affinity and loop time, the repulsion's pair rate, the attraction's byte rate (the loop with the CSR against the same
loop with an empty one: the repulsion is branch-free, so the difference is the attraction), and both paths' KL at 8192."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tacorl_amd import ops  # noqa: E402

DEV = "cuda:0"
N_ITER, REPEATS, D, PERPLEXITY = 1000, 5, 16, 40.0
# what the force pass is set against (measured on an MI355X: a float4 copy out of HBM; an Infinity-Cache resident table; rows
# shared through an XCD's L2)
HBM_TBS, MALL_TBS, L2_TBS = 6.29, 8.6, 16.8
FMA_PEAK = 157.3e12 / 2  # fp32 vector FMA per second (the spec's 157.3 TFLOPS)
NBR_REPEATS = 3
CALLBACK_NOTE = ("The `tsne callback` line is `test_callbacks_through_minitrainer_on_playlmp`'s: its per-epoch KLs are the "
                 "PlayLMP's training losses, and its map embeds plans that the module samples from torch's global generator, "
                 "which that test does not seed.  Its figures record one run and depend on the generator's state when the test "
                 "starts; they are no property of the t-SNE kernels, whose bits below the dense cap are held by "
                 "`test_tsneplot_below_the_cap_is_tsne_embed`.")


def table(N):
    g = torch.Generator(device="cpu").manual_seed(N)
    centres = torch.rand(12, D, generator=g) * 1.6 - 0.8
    X = torch.tanh(centres[torch.randint(0, 12, (N,), generator=g)] + 0.15 * torch.randn(N, D, generator=g))
    return X.to(DEV), (1e-4 * torch.randn(N, 2, generator=g)).to(DEV)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def hip_affinities(X):
    return ops.tsne_affinities(X, PERPLEXITY)


def hip_loop(P, Y0, ws):
    Y, u, g = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(N_ITER):
        early = it < 250
        ops.tsne_step(P, Y, u, g, 12.0 if early else 1.0, 0.5 if early else 0.8, 200.0, ws)
    return Y


def torch_affinities(X):
    N = X.shape[0]
    xc = X - X.mean(0)
    xn = xc / xc.abs().max()
    d = torch.cdist(xn, xn).square_()
    eye = torch.eye(N, dtype=torch.bool, device=X.device)
    d.masked_fill_(eye, float("inf"))
    t = d - d.min(1, keepdim=True).values
    t0 = t.masked_fill(eye, 0)
    beta = torch.ones(N, 1, device=X.device)
    lo, hi = torch.zeros_like(beta), torch.full_like(beta, float("inf"))
    target = torch.log(torch.tensor(PERPLEXITY, device=X.device))
    for step in range(200):
        e = torch.exp(-beta * t)
        S = e.sum(1, keepdim=True)
        H = torch.log(S) + beta * (e * t0).sum(1, keepdim=True) / S
        diff = H - target
        done = diff.abs() < 1e-5
        if step % 10 == 9 and bool(done.all()):
            break
        up = (diff > 0) & ~done
        dn = (diff <= 0) & ~done
        lo, hi = torch.where(up, beta, lo), torch.where(dn, beta, hi)
        beta = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2),
                           torch.where(dn, torch.where(lo == 0, beta / 2, (beta + lo) / 2), beta))
    c = torch.exp(-beta * t) / S
    return (c + c.T) / (2 * N)


def torch_loop(P, Y0):
    Y, u, g = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(N_ITER):
        ex, mom = (12.0, 0.5) if it < 250 else (1.0, 0.8)
        s = (Y * Y).sum(1)
        w = 1.0 / (1.0 + (s[:, None] + s[None, :] - 2.0 * (Y @ Y.T)).clamp_min_(0))
        w.fill_diagonal_(0)
        Z = w.sum()
        pw = P * w
        attr = pw.sum(1, keepdim=True) * Y - pw @ Y
        w.mul_(w)
        rep = w.sum(1, keepdim=True) * Y - w @ Y
        grad = 4.0 * (ex * attr - rep / Z)
        g = torch.where((grad > 0) != (u > 0), g + 0.2, g * 0.8).clamp_min_(0.01)
        u = mom * u - 200.0 * (g * grad)
        Y = Y + u
        Y = Y - Y.mean(0)
    return Y


def measure(N):
    X, Y0 = table(N)
    P, _, status, ws = hip_affinities(X)      # warm-up of both paths at this shape
    hip_loop(P, Y0, ws)
    Pt = torch_affinities(X)
    torch_loop(Pt, Y0)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0], status
    rel = float((P - Pt).abs().max() / Pt.max())
    rows = {k: [] for k in ("hip_aff", "hip_loop", "torch_aff", "torch_loop")}
    for _ in range(REPEATS):                   # alternating, so that a busy neighbour hits both alike
        rows["hip_aff"].append(timed(lambda: hip_affinities(X))[0])
        rows["hip_loop"].append(timed(lambda: hip_loop(P, Y0, ws))[0])
        rows["torch_aff"].append(timed(lambda: torch_affinities(X))[0])
        rows["torch_loop"].append(timed(lambda: torch_loop(Pt, Y0))[0])
    med = {k: statistics.median(v) for k, v in rows.items()}
    spread = {k: (min(v), max(v)) for k, v in rows.items()}
    return med, spread, rel


def nbr_loop(csr, Y0, ws):
    Y, u, g = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(N_ITER):
        early = it < 250
        ops.tsne_nbr_step(*csr, Y, u, g, 12.0 if early else 1.0, 0.5 if early else 0.8, 200.0, ws)
    return Y


def measure_nbr(N):
    """{aff, loop, loop_empty: (median, min, max) ms; nnz; kl; and at N <= TSNE_MAX_N the dense path's aff, loop, kl}."""
    X, Y0 = table(N)
    a = ops.tsne_nbr_affinities(X, PERPLEXITY)  # warm-up of the shape
    csr, ws = (a["row_ptr"], a["col"], a["val"]), a["ws"]
    empty = (torch.zeros_like(a["row_ptr"]), a["col"], a["val"])
    Y = nbr_loop(csr, Y0, ws)
    torch.cuda.synchronize()
    assert a["status"].tolist() == [0, 0], a["status"]
    out = {"nnz": int(a["row_ptr"][N]), "kl": float(ops.tsne_nbr_kl(*csr, Y, ws).item())}
    rows = {"aff": [], "loop": [], "loop_empty": []}
    dense = N <= ops.TSNE_MAX_N
    if dense:
        P, _, _, wsd = hip_affinities(X)
        out["dense_kl"] = float(ops.tsne_kl(P, hip_loop(P, Y0, wsd), wsd).item())
        rows.update(dense_aff=[], dense_loop=[])
    for _ in range(NBR_REPEATS):
        rows["aff"].append(timed(lambda: ops.tsne_nbr_affinities(X, PERPLEXITY, ws=ws))[0])
        rows["loop"].append(timed(lambda: nbr_loop(csr, Y0, ws))[0])
        rows["loop_empty"].append(timed(lambda: nbr_loop(empty, Y0, ws))[0])
        if dense:
            rows["dense_aff"].append(timed(lambda: hip_affinities(X))[0])
            rows["dense_loop"].append(timed(lambda: hip_loop(P, Y0, wsd))[0])
    out.update({k: (statistics.median(v), min(v), max(v)) for k, v in rows.items()})
    return out


def nbr_section(sizes):
    out = ["## Neighbour-sparse path (above 8192 plans)", "",
           f"D = {D}, perplexity {PERPLEXITY:g} (K = {ops.tsne_nbr_k(PERPLEXITY)}), {N_ITER} iterations; HIP events, one warm-up run per shape, "
           f"median of {NBR_REPEATS} (min .. max), milliseconds.  `dense` is the exact path of the section above on the same table "
           "(N <= 8192 only).  Pair rate: N (N - 1) pairs per iteration over the loop time with an EMPTY CSR (repulsion, fold and "
           f"update only), as a share of the {FMA_PEAK / 1e12:.1f} T fp32 FMA/s vector peak - one pair per FMA slot would be 100 %; a pair "
           "is about 20 vector instructions here, an IEEE division among them, so the ceiling of this formulation is near 5 %.  "
           "Attraction: 16 B per stored entry (column, value, the gathered y) over the loop time with the CSR minus the loop time "
           f"without it, against the {HBM_TBS} TB/s of a float4 copy out of HBM.", "",
           "| N | stored entries | affinities | loop | loop, empty CSR | pair rate | attraction | KL | dense: affinities | dense: loop | dense: KL |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for N in sizes:
        m = measure_nbr(N)
        f = lambda k: f"{m[k][0]:.2f} ({m[k][1]:.2f} .. {m[k][2]:.2f})" if k in m else "-"  # noqa: E731
        pairs = N * (N - 1) / (m["loop_empty"][0] * 1e-3 / N_ITER)
        dt = (m["loop"][0] - m["loop_empty"][0]) * 1e-3 / N_ITER
        attr = f"{m['nnz'] * 16 / dt / 1e12:.2f} TB/s = {100 * m['nnz'] * 16 / dt / 1e12 / HBM_TBS:.0f} %" if dt > 0 else "(below the spread)"
        out.append(f"| {N} | {m['nnz']} | {f('aff')} | {f('loop')} | {f('loop_empty')} | {pairs / 1e12:.2f} T pairs/s = "
                   f"{100 * pairs / FMA_PEAK:.1f} % | {attr} | {m['kl']:.4f} | {f('dense_aff')} | {f('dense_loop')} | "
                   + (f"{m['dense_kl']:.4f} |" if "dense_kl" in m else "- |"))
        print(out[-1], flush=True)
        whole = (m["aff"][0] + m["loop"][0]) / 1e3
    return out + ["", f"The whole map at N = {sizes[-1]} takes {whole:.1f} s, once per validation epoch, against the minutes a host "
                  "Barnes-Hut run needs at that size and the hours of the epoch it follows: `TSNEPlot(max_points=None)` keeps the "
                  "kernel's cap as its default.  The two KLs at 8192 are costs of two different P (the dense one has every pair, "
                  "the sparse one the neighbour pairs only) and are not comparable as numbers.", ""]


def test_lines():
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_tsne_gpu.py"),
                        os.path.join(ROOT, "tests", "test_tsne_nbr_gpu.py"), "-q", "-s", "-p",
                        "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "(no output)"
    return [ln.lstrip(".F") for ln in r.stdout.splitlines() if re.match(r"^[.F]*tsne ", ln)], tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne.md"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096, 8192])
    ap.add_argument("--nbr-sizes", type=int, nargs="*", default=[8192, 32768, 131072])
    ap.add_argument("--no-tests", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/tsne_md.py needs a GPU"
    out = ["# t-SNE of latent plans, exact and neighbour-sparse: bound use and time", "",
           f"Written by `tools/tsne_md.py` on {torch.cuda.get_device_name(0)}.  Definitions: `include/tacorl_hip.h`; kernels: "
           "`tacorl_amd/csrc/tsne_ops.hip`; yardsticks: the fp64 restatements `tests/tsne_ref.py` and `tests/tsne_nbr_ref.py`.", ""]
    out += ["## Time", "",
            f"D = {D}, perplexity {PERPLEXITY:g}, {N_ITER} iterations; HIP events, one warm-up run per shape, median of {REPEATS} "
            "(min .. max), milliseconds.  `torch ops` is the same definition in dense torch operations on the same GPU - the "
            "baseline, not the code under test.  Force pass: the N^2 * 4 B of P one iteration reads, over loop time / "
            f"{N_ITER} (the update launch included), against the rates measured for this GPU model: {HBM_TBS} TB/s for a float4 "
            f"copy out of HBM, {MALL_TBS} TB/s for an Infinity-Cache resident table, {L2_TBS} TB/s for rows shared through an "
            "XCD's L2.  P is 4 / 64 / 256 MiB at N = 1024 / 4096 / 8192: inside the L2s' 32 MiB only at N = 1024, where the "
            "iteration is its two launches, so no size runs at an L2 rate.", "",
            "| N | affinities: kernels | affinities: torch ops | loop: kernels | loop: torch ops | whole: kernels / torch | "
            "force pass | max abs P difference / max P |", "|---|---|---|---|---|---|---|---|"]
    slower = []
    for N in a.sizes:
        med, sp, rel = measure(N)
        f = lambda k: f"{med[k]:.2f} ({sp[k][0]:.2f} .. {sp[k][1]:.2f})"  # noqa: E731
        whole_h, whole_t = med["hip_aff"] + med["hip_loop"], med["torch_aff"] + med["torch_loop"]
        tbs = N * N * 4 / (med["hip_loop"] * 1e-3 / N_ITER) / 1e12
        out.append(f"| {N} | {f('hip_aff')} | {f('torch_aff')} | {f('hip_loop')} | {f('torch_loop')} | {whole_h:.1f} / {whole_t:.1f} = "
                   f"{whole_h / whole_t:.3f} | {tbs:.2f} TB/s = {100 * tbs / HBM_TBS:.0f} % of the HBM copy rate | {rel:.2e} |")
        for part in ("aff", "loop"):
            if med["hip_" + part] > med["torch_" + part]:
                slower.append((N, part, med["hip_" + part], med["torch_" + part]))
        print(out[-1], flush=True)
    out += [""] + ([f"The kernel path is SLOWER than the torch-op statement at: {slower}"] if slower else
                   ["The kernel path is faster than the torch-op statement in both parts at every size."]) + [""]
    if a.nbr_sizes:
        out += nbr_section(a.nbr_sizes)
    if not a.no_tests:
        lines, tail = test_lines()
        out += ["## Bound use and trajectory deviations (tests/test_tsne_gpu.py, tests/test_tsne_nbr_gpu.py)", "", f"pytest: `{tail}`", "", CALLBACK_NOTE, "", "```"] + lines + ["```", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
