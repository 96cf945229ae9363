"""profiles/dr3_margins.md from the margins that tests/test_dr3_kernel_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_dr3_kernel_gpu.py -s
    python tools/dr3_margins_md.py margins.jsonl profiles/dr3_margins.md

(one JSON line per (shape, quantity), tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import json
import os
import re
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if "test_dr3_kernel_gpu" in r["test"] and r["kind"].startswith("dr3 kernel")]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"

table = {}
for r in rows:
    m = re.match(r"B(\d+) Eo(\d+) ld(\d+) gs([\d.]+): (.+)", r["tensor"])
    B, Eo, ld, gs, what = int(m[1]), int(m[2]), int(m[3]), float(m[4]), m[5]
    table.setdefault((B, Eo, ld, gs), {})[what] = r["err"]

out = ["# tacorl_dr3_fwd_bwd against fp64: measured margins\n"]
out.append("Formatted by `tools/dr3_margins_md.py` from the margins ONE run of `tests/test_dr3_kernel_gpu.py` recorded\n"
           "(`golden_util.record_margin`); the numbers are that run's, not a distribution, and no bound of the tests is taken from\n"
           "them.  Measured on: " + box + ".  The fp64 references are CPU evaluations of `tests/dr3_ref.py`.\n")
out.append("`error / bound` = worst `|got - fp64| / bound` over both critics of the launch; 1.0 is the bound.  Value: bound =\n"
           "(B Eo + 2) 2^-24 coef / B sum |obs next|.  Gradient element: bound = 3 2^-24 (|d_before| + |coef gs / B next|), worst\n"
           "element of the (B, Eo) rows.  coef = 0.03; `ld` = leading dimension of the operand and gradient rows.\n")
out.append("| B | Eo | ld | gs | error / bound, value | error / bound, gradient element |")
out.append("|---|---|---|---|---|---|")
for (B, Eo, ld, gs), row in sorted(table.items()):
    out.append(f"| {B} | {Eo} | {ld} | {gs:g} | {row.get('value', float('nan')):.3g} | {row.get('gradient element', float('nan')):.3g} |")
out.append("\nThe add into the q_loss slot, the untouched columns >= Eo, the two-run comparison and the refusals are exact comparisons:\n"
           "they pass or fail, there is no margin.")
over = [r for r in rows if r["err"] > r["tol"]]
out.append(f"\nEntries over their bound: {len(over)}" + "".join(f"\n- {r['tensor']}: {r['err']:.3g}" for r in over) + "\n")
open(OUT, "w").write("\n".join(out) + "\n")
