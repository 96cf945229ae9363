"""profiles/pr_forward_margins.md from the margins that tests/test_pr_fp64_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_pr_fp64_gpu.py -s
    python tools/pr_margins_md.py margins.jsonl profiles/pr_forward_margins.md

(one JSON line per comparison, tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import collections
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import pr_ref as R  # noqa: E402

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if 'test_pr_fp64_gpu' in r['test']]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"


def of(kind):
    return [r for r in rows if r['kind'] == kind]


out = []
out.append("# One-launch plan-recognition forward against fp64: measured margins\n")
out.append("Formatted by `tools/pr_margins_md.py` from the margins ONE run of `tests/test_pr_fp64_gpu.py` recorded\n"
           "(`golden_util.record_margin`); the numbers are that run's, not a distribution.  Measured on: " + box + ".\n"
           "The fp64 references, the population levels and fp32 torch's errors are CPU evaluations of `tests/pr_ref.py` on that box's\n"
           "host.  Every bound is stated in `tests/pr_ref.py`; `tests/test_pr_ref_cpu.py` shows that each is at least "
           f"{R.FAULT_RATIO:g} x below the planted faults.\n")

out.append("## S: d_model 32, train-mode launch, every saved tensor on the kernel's own saved input\n")
out.append("Worst `|got - ref| / bound` over every element; 1.0 is the bound.  Where each bound comes from:\n\n"
           f"- `qkv`, `proj`, `ff1`: `lin_bound`, {R.C_SUM:g} K' 2^-24 (sum |x~||w~| + |b|), K' = 33 (32 terms and the bias), operands the bf16 RNE of the saved input;\n"
           f"- `ff2`: the same with K' = `ffn2_terms` = 256 ceil(chunks / 4) + 4: a wave's chunks in one accumulator started at b2, three adds to join;\n"
           "- `att`: `att_bound`, ((4 hd + 12) Lam + 2 T + 8) 2^-24 sum p |v|, Lam = the query's largest sum |q k| / sqrt(hd), exp2 and the reciprocal at 1 ulp;\n"
           "- `x1`, `st1`, `st2`, `xin` of the next layer: `ln_bound`, the roundings of the residual add, the two sums (depth D / 4 + 1), rstd and the affine map, counted;\n"
           "- `pooled`: the time mean of the LayerNorm-2 reference, its bound averaged plus "
           f"{R.C_SUM:g} T 2^-24 mean |y| (`pool_bound`).\n\n"
           "`xin0 = emb + pos`, the guard tails, the untouched head / plan buffers and the bf16 mirror are bit comparisons.\n")
s = collections.OrderedDict()
for r in of("S err / bound"):
    w = r['tensor'].split(' ')
    s.setdefault(" ".join(w[:-1]), []).append((w[-1], r['err']))
groups = ("qkv", "att", "proj", "x1", "st1", "ff1", "ff2", "st2", "xin", "pooled")
out.append("| case (T, FF, L, B, ld_emb) | " + " | ".join(groups) + " |")
out.append("|---|" + "---|" * len(groups))
for c, sts in s.items():
    worst = {g: max([e for n, e in sts if n.split('[')[0] == g] + [0.0]) for g in groups}
    out.append(f"| {c} | " + " | ".join(f"{worst[g]:.2g}" if any(n.split('[')[0] == g for n, _ in sts) else "-" for g in groups) + " |")
out.append("\n(the worst layer of each tensor.)  I: the inference launch's `pooled` equals the train launch's bit for bit at every case.\n")

out.append("## H: head and plan of the _sample launches from the kernel's own pooled / head\n")
out.append(f"`head`: {R.C_SUM:g} (D + 1) 2^-24 (sum |Wc||pooled| + |bc|) on the kernel's own fp32 (Wc, bc, pooled).  `plan`: {R.ACT_FACTOR:g} x the worst error of\n"
           "plain fp32 torch on the same head and eps and on the reference's population (`sample_level`; in brackets), at least one fp32\n"
           "ulp of the value.  Every case holds var_raw above 20 and below -20.\n")
h = collections.OrderedDict()
for r in of("H err / bound"):
    w = r['tensor'].split(' ')
    h.setdefault(" ".join(w[:3]), []).append((w[3], w[4], r['err'], r['floor']))
out.append("| case | err / bound |")
out.append("|---|---|")
for c, sts in h.items():
    out.append(f"| {c} | " + ", ".join(f"{e} {n} {v:.2g}" + (f" ({fl:.1e})" if fl is not None else "") for e, n, v, fl in sts) + " |")

out.append("\n## C: tacorl_pr_head_compose\n")
out.append(f"`Wc` against fp64 W_head W_fc at {R.C_SUM:g} FC 2^-24 sum |w_head||w_fc|, `bc` against W_head b_fc + b_head at {R.C_SUM:g} (FC + 1) 2^-24 (sum + |b_head|).\n")
c_ = collections.OrderedDict()
for r in of("C err / bound"):
    w = r['tensor'].split(' ')
    c_.setdefault(" ".join(w[:3]), {})[w[3]] = r['err']
out.append("| case | Wc | bc |")
out.append("|---|---|---|")
for c, d in c_.items():
    out.append(f"| {c} | {d.get('Wc', 0):.2g} | {d.get('bc', 0):.2g} |")

out.append("\n## E2: d_model 64, per-sequence error of pooled against the fully rounded fp64 forward\n")
out.append(f"bound = {R.E2E_FACTOR:g} x the level; level = the median (for the lower quartile of the launch) and the maximum (for its worst sequence) of\n"
           f"the fp32 rounded restatement's own per-sequence error over {R.POP} seeded sequences (`e2e_levels`).\n")
out.append("| case | figure | measured | level | bound |")
out.append("|---|---|---|---|---|")
for r in of("E2 per sequence"):
    w = r['tensor'].split(' ')
    out.append(f"| {' '.join(w[:5])} | {' '.join(w[5:])} | {r['err']:.2e} | {r['floor']:.2e} | {r['tol']:.2e} |")
out.append("\nE1 (a sequence's pooled row alone, first, last and in a batch of another size; the sample launch's pooled; both d_model) and R\n"
           "(refusals) are bit-exact or return-code comparisons: they pass or fail, there is no margin.")
over = [r for r in rows if r['tol'] and r['err'] > r['tol']]
out.append(f"\nEntries over their bound: {len(over)}" + ("".join(f"\n- {r['tensor']} ({r['kind']}): {r['err']:.3g} > {r['tol']:.3g}" for r in over)) + "\n")
open(OUT, 'w').write("\n".join(out) + "\n")
