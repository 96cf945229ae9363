"""profiles/mlp_margins.md from the margins that tests/test_mlp_fp64_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_mlp_fp64_gpu.py -s
    python tools/mlp_margins_md.py margins.jsonl profiles/mlp_margins.md

(one JSON line per comparison, tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import collections
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mlp_ref as R  # noqa: E402

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if 'test_mlp_fp64_gpu' in r['test']]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"


def of(kind):
    return [r for r in rows if r['kind'] == kind]


def case(r, extra):
    """'path site rows mode ...' -> ((path, site, rows, mode), the last `extra` words)."""
    w = r['tensor'].split(' ')
    return tuple(w[:4]), w[4:4 + extra]


out = []
out.append("# Fused MLP chain against fp64: measured margins\n")
out.append("Formatted by `tools/mlp_margins_md.py` from the margins ONE run of `tests/test_mlp_fp64_gpu.py` recorded\n"
           "(`golden_util.record_margin`); the numbers are that run's, not a distribution.  Measured on: " + box + ".\n"
           "The fp64 references, the oracle's levels and fp32 torch's activation errors are CPU evaluations of `tests/mlp_ref.py` and\n"
           "`oracle/tacorl_oracle.py` on that box's host.\n\n"
           "Paths: `save` = `tacorl_mlp_fwd_fused` / `_bwd_fused_dgrad` / `_bwd_fused_wgrad` with every activation saved (the few-row\n"
           "kernels; 128 / 64-row workgroups from 2048 rows on), `lean` = the same entry points in lean mode (from 2048 rows on the\n"
           "many-row kernels with bf16 y / fp16 act' / bf16 dZ saves where the site has them: 32-row workgroups, persistent from 16384\n"
           "rows on), `lean_pers0` = the per-block 128 / 64-row kernels (`TACORL_MLP_PERS = TACORL_MLP_PERS_BWD = 0`), `layer_bf16` /\n"
           "`layer_f32` = `tacorl_mlp_fwd` / `tacorl_mlp_bwd` per layer.  Sites: "
           + ", ".join(f"`{s}` {d} acts {a} ld {ld}" for s, (d, a, ld) in R.SITES.items()) + ".\n"
           "Modes: `mixed` = a second problem of 130 rows in the same call, `two` = a second problem of rows - 4000, `one` = alone.\n")

out.append("## F1: every saved activation, element by element, on the kernel's own saved input\n")
out.append(f"Worst `|got - ref| / bound` over every element of every problem of the call; 1.0 is the bound.  `z` = a saved pre-activation:\n"
           f"bound = {R.C_SUM:g} K 2^-24 (sum |x||w| + |b|).  `a` = the saved output against act(saved z): {R.ACT_FACTOR:g} x the worst error of plain fp32\n"
           "torch on the same z (in brackets), at least one fp32 ulp of the value.  `y` = an output whose z is not saved (ReLU, NONE, TANH;\n"
           "bf16 y of the many-row saves: + 1 bf16 ulp): the sum's bound x the activation's Lipschitz constant + the activation's\n"
           "tolerance.  `s` = fp16 act' of the many-row saves (+ 1 fp16 ulp).  A few-row lean call saves no hidden output: its z and\n"
           "output are compared bit for bit with the saving mode instead and have no entry here.\n")
f1 = collections.OrderedDict()
for r in of("F1 err / bound"):
    c, (st,) = case(r, 1)
    f1.setdefault(c, []).append((st, r['err'], r['floor']))
out.append("| path | site | rows | mode | err / bound per stage |")
out.append("|---|---|---|---|---|")
for c, sts in f1.items():
    out.append("| " + " | ".join(c) + " | " + ", ".join(f"{s} {e:.2g}" + (f" ({fl:.1e})" if fl is not None else "") for s, e, fl in sts) + " |")

out.append("\n## F2: every output row against the fully rounded reference\n")
out.append(f"Relative error of the worst row (denominator floored at the RMS row norm).  bound = {R.E2E_FACTOR:g} x the level; level = the fp32\n"
           "rounded oracle's worst row over every site at the pooled row counts " + str(R.LEVEL_ROWS) + " of the problem's bucket (< 64 rows /\n"
           "more) and on the problem itself (`mlp_ref.grad_bounds`).\n")
out.append("| path | site | rows | mode | problem | worst row | level | bound |")
out.append("|---|---|---|---|---|---|---|---|")
for r in of("F2 per row"):
    c, (pi, _) = case(r, 2)
    out.append("| " + " | ".join(c) + f" | {pi[1:]} | {r['err']:.2e} | {r['floor']:.2e} | {r['tol']:.2e} |")

out.append("\n## B1 / B2: gradients by slice against fp64\n")
out.append(f"Worst slice of a class over the problems and layers of the call: `error / bound (level)`.  Classes: d_x per row, dW per output\n"
           f"neuron, db per 16 elements.  bound = {R.GRAD_FACTOR:g} x the level, level = the fp32 rounded oracle's autograd error on the class, pooled as\n"
           "in F2 (`layer_f32`: the oracle without operand rounding on the same problem, at least 16 x 2^-24).  d_x is not asked for where\n"
           "rows % 4 == 0; the second problem has no parameter gradients where rows is odd.\n")
b = collections.OrderedDict()
for r in of("B gradient slices"):
    c, (cls,) = case(r, 1)
    b.setdefault(c, {})[cls] = r
out.append("| path | site | rows | mode | " + " | ".join(R.CLASSES) + " |")
out.append("|---|---|---|---|" + "---|" * len(R.CLASSES))
for c, d in b.items():
    out.append("| " + " | ".join(c) + " | " + " | ".join(
        f"{d[k]['err']:.1e} / {d[k]['tol']:.1e} ({d[k]['floor']:.1e})" if k in d else "-" for k in R.CLASSES) + " |")

acc = of("B2 accumulate err / bound")
out.append("\n## B2: accumulate = 1\n")
out.append(f"The accumulating call on a seeded base against fp32(base + the plain call's gradient), per element, bound = one fp32 rounding\n"
           f"of the sum (2^-23 |sum|): worst use over the {len(acc)} (call, problem) pairs: {max([r['err'] for r in acc] + [0.0]):.3g}"
           " (0 = bit-identical to the sum).\n")

out.append("## B3: grad(A u B) = grad(A) + grad(B)\n")
out.append(f"Worst element of any weight or bias gradient, `|difference| / bound`.  bound = min({R.C_SUM:g} M, {R.C_SUM:g} x {R.ADD_LAMBDA:g} sqrt(M)) 2^-24 sum|terms|\n"
           f"(`mlp_ref.additivity_bound`); worst case = {R.C_SUM:g} M 2^-24 sum|terms| alone.\n")
wc = {r['tensor']: r['err'] for r in of("B3 additivity err / worst-case bound")}
out.append("| site | rows | worst | of the worst-case bound | in |")
out.append("|---|---|---|---|---|")
for r in of("B3 additivity err / bound"):
    s, m, name = r['tensor'].split(' ')
    out.append(f"| {s} | {m} | {r['err']:.2g} | {wc[r['tensor']]:.2g} | `{name}` |")
out.append("\nF3 (same rows, same bits wherever they are served; the gathered forward), the batched preparation / reduces and B4 (refusals)\n"
           "are bit-exact or return-code comparisons: they pass or fail, there is no margin.")
over = [r for r in rows if r['tol'] and r['err'] > r['tol']]
out.append(f"\nEntries over their bound: {len(over)}" + ("".join(f"\n- {r['tensor']} ({r['kind']}): {r['err']:.3g} > {r['tol']:.3g}" for r in over)) + "\n")
open(OUT, 'w').write("\n".join(out) + "\n")
