"""profiles/encoder_margins.md from the margins that tests/test_encoder_fp64_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_encoder_fp64_gpu.py -s
    python tools/encoder_margins_md.py margins.jsonl profiles/encoder_margins.md

(one JSON line per comparison, tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import collections
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import encoder_ref as R  # noqa: E402

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if 'test_encoder_fp64_gpu' in r['test']]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"


def of(kind):
    return [r for r in rows if r['kind'] == kind]


out = []
out.append("# Image encoder against fp64: measured margins\n")
out.append("Formatted by `tools/encoder_margins_md.py` from the margins ONE run of `tests/test_encoder_fp64_gpu.py` recorded\n"
           "(`golden_util.record_margin`); the numbers are that run's, not a distribution.  Measured on: " + box + ".\n"
           "The fp64 references, the oracle's levels and the floors are CPU evaluations of `tests/encoder_ref.py` and\n"
           "`oracle/tacorl_oracle.py` on that box's host.  Paths: `fused` = `tacorl_encoder_fwd_fused` / `tacorl_encoder_bwd_fused`\n"
           "(150x200: `encoder_ring.hip` forward), `generic_bf16` / `generic_f32` = `tacorl_encoder_fwd` / `tacorl_encoder_bwd` per layer.\n"
           f"Inputs: `encoder_ref.images` (structured, exact in bf16), soft-argmax temperature {R.T_PEAKED} (C5: {R.T_SHARP}).\n")

out.append("## C1 / C2: every saved activation, element by element, on the kernel's own saved input\n")
out.append(f"Worst `|got - ref| / bound` over every element of every problem; 1.0 is the bound.  bound = {R.C_SUM:g} K 2^-24 (sum |x||w| + |b|)\n"
           "(K terms: 193 / 513 / 577 for the convolutions, 129 / 257 for the FC layers), plus one bf16 ulp of |ref| for y1 / y2 of the\n"
           "fused path, which stores them as bf16: there the ratio is the stored rounding, at most half an ulp.\n")
c1 = collections.OrderedDict()
for r in of("C1 err / bound"):
    g, pth, st = r['tensor'].split(' ')
    c1.setdefault((g, pth), {})[st] = r['err']
out.append("| geometry | path | y1 | y2 | y3 | fc1 | out |")
out.append("|---|---|---|---|---|---|---|")
for (g, pth), d in c1.items():
    out.append(f"| {g} | {pth} | " + " | ".join("%.2g" % d[s] for s in ("y1", "y2", "y3", "fc1", "out")) + " |")

for sec, title in (("C1", "## C1 / C2: soft-argmax keypoints (pixels)\n"), ("C5", f"## C5: soft-argmax at temperature {R.T_SHARP} (logits past exp's fp32 range)\n")):
    out.append("\n" + title)
    out.append(f"Worst keypoint of the worst problem.  bound = max({R.SA_FACTOR:g} x the worst error of plain fp32 torch on the same y3, floor),\n"
               "floor = 2^-24 max|logit| max(h, w).\n")
    fl = {r['tensor']: r['err'] for r in of(sec + " soft-argmax floor")}
    out.append("| geometry | path | kernel error | fp32 torch error | floor | bound | error / bound |")
    out.append("|---|---|---|---|---|---|---|")
    for r in of(sec + " soft-argmax"):
        g, pth, _ = r['tensor'].split(' ')
        out.append(f"| {g} | {pth} | {r['err']:.2e} | {r['floor']:.2e} | {fl[r['tensor']]:.2e} | {r['tol']:.2e} | {r['err'] / r['tol']:.2g} |")

out.append("\n## C3: every image's output against the end-to-end reference\n")
out.append(f"Relative error of the worst image's 32-vector.  bound = {R.E2E_FACTOR:g} x the fp32 rounded oracle's worst image over every forward\n"
           "problem of every geometry (`encoder_ref.e2e_level`: a bf16 operand that rounds the other way is a chance event per image).\n")
out.append("| geometry | path | worst image | oracle's worst image at this geometry | bound |")
out.append("|---|---|---|---|---|")
for r in of("C3 per image"):
    g, pth = r['tensor'].split(' ')
    out.append(f"| {g} | {pth} | {r['err']:.2e} | {r['floor']:.2e} | {r['tol']:.2e} |")

out.append("\n## D1: gradients by slice against fp64\n")
out.append(f"Worst slice of a tensor class (weights per output channel, conv weights per kernel tap, biases, temperature) over the problems:\n"
           f"`error / bound (the oracle's level at this geometry)`.  bound = {R.GRAD_FACTOR:g} x the class's level over every geometry\n"
           f"(`encoder_ref.grad_levels`), level = the fp32 oracle's autograd error on the same slices; temperature: at least {R.FLOOR_FACTOR:g} x\n"
           "`golden_util.gradient_floor`; accumulate = 1 adds the rounding of the accumulation itself.  ReLU gates that fp32 cannot decide\n"
           "(pre-activation within the C1 bound of zero) are the forward kernel's in the reference.\n")
d1 = collections.OrderedDict()
for r in of("D1 gradient slices"):
    g, pth, acc, cls = r['tensor'].split(' ')
    d1.setdefault((g, pth, acc[-1]), {})[cls] = r
CLS = ["weight/channel", "weight/tap", "bias", "temperature"]
out.append("| geometry | path | accumulate | " + " | ".join(CLS) + " |")
out.append("|---|---|---|" + "---|" * len(CLS))
for (g, pth, acc), d in d1.items():
    out.append(f"| {g} | {pth} | {acc} | " + " | ".join(f"{d[c]['err']:.1e} / {d[c]['tol']:.1e} ({d[c]['floor']:.1e})" for c in CLS) + " |")

out.append("\n## D2: grad(A u B) = grad(A) + grad(B)\n")
out.append(f"Worst element of any gradient, `|difference| / bound`, bound = {R.C_SUM:g} n 2^-24 sum|terms| (n = images x output pixels).\n")
out.append("| geometry | path | worst | in |")
out.append("|---|---|---|---|")
for r in of("D2 additivity err / bound"):
    g, pth, name = r['tensor'].split(' ')
    out.append(f"| {g} | {pth} | {r['err']:.2g} | `{name}` |")
out.append("\nC4 (same image, same bits wherever it is served) and D3 (the split entry points equal the composite) are bit-exact comparisons:\n"
           "they pass or fail, there is no margin.")
open(OUT, 'w').write("\n".join(out) + "\n")
