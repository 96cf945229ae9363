"""profiles/ring_margins.md from the margins that tests/test_ring_fp64_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_ring_fp64_gpu.py -s
    python tools/ring_margins_md.py margins.jsonl profiles/ring_margins.md

(one JSON line per (test, entry, route), tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ring_ref as R  # noqa: E402

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if 'test_ring_fp64_gpu' in r['test'] and r['kind'] == "ring err / bound"]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"

worst = {}
for r in rows:
    entry, tile, tmap, cls, shape = r['tensor'].split('|')
    row = worst.setdefault((entry, tile, tmap), {"gates": 0})
    row["gates"] += int(r['floor'] or 0)
    if cls not in row or r['err'] > row[cls][0]:
        row[cls] = (r['err'], shape)

out = ["# Ring GEMM and its weight gradients against fp64: measured margins\n"]
out.append("Formatted by `tools/ring_margins_md.py` from the margins ONE run of `tests/test_ring_fp64_gpu.py` recorded\n"
           "(`golden_util.record_margin`); the numbers are that run's, not a distribution, and no tolerance of the tests is taken from\n"
           "them.  Measured on: " + box + ".  The fp64 references are CPU evaluations of `tests/ring_ref.py` on that box's host.\n")
out.append(f"`err / bound` = worst `|got - ref| / bound` over every element of every launch of the row; 1.0 is the bound; `sum`: outputs with\n"
           f"act none / ReLU and the weight gradients, `SiLU / Tanh`: outputs behind those activations, each with the shape of its worst value;\n"
           f"bound = {R.C_SUM:g} n 2^-24 (sum |x||w| + |b| + |b2| + |addend|) with n the number of terms (weight gradients: n = R reduction rows;\n"
           f"accumulate = 1: + one fp32 rounding of the sum); SiLU / Tanh outputs add {R.ACT_FACTOR:g} x plain fp32 torch's error on the same z.\n"
           f"`gates` = ReLU elements whose |z| lies within the bound of zero, summed over the row's launches (cap: {100 * R.GATE_CAP:g} % of an output;\n"
           "G4's row: placements of the probe row whose bits differ).  Shapes:\n"
           "forward entries (M, K, N) or (nprob, M, M2, K, N[, extension]); `ld` (nprob, M, K, N, ldx, ldy, problem); weight gradients\n"
           "(R, M, N).  Weight-gradient rows name the tile map in the route column and dW / db in the map column.\n")
out.append("| entry | route | map | err / bound, sum | at | err / bound, SiLU / Tanh | at | gates |")
out.append("|---|---|---|---|---|---|---|---|")
cell = lambda row, c: f"{row[c][0]:.3g} | {row[c][1]}" if c in row else "- | -"  # noqa: E731
for (entry, tile, tmap), row in sorted(worst.items()):
    out.append(f"| `{entry}` | {tile} | {tmap} | {cell(row, 'sum')} | {cell(row, 'act')} | {row['gates']} |")
out.append("\nThe bf16 copies (bit-equal to bf16(y)), G4 (one row, one bit pattern), W2 (the batched launch against single launches), W3 (the\n"
           "slabs form against the fp32 sum of single launches) and the refusals are exact comparisons: they pass or fail, there is no margin.")
over = [r for r in rows if r['err'] > r['tol']]
out.append(f"\nEntries over their bound: {len(over)}" + "".join(f"\n- {r['tensor']}: {r['err']:.3g}" for r in over) + "\n")
open(OUT, 'w').write("\n".join(out) + "\n")
