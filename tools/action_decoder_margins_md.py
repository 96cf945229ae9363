"""profiles/action_decoder_module_margins.md from the margins that tests/test_action_decoder_gpu.py records:

    TACORL_MARGINS=margins.jsonl python -m pytest -m gpu tests/test_action_decoder_gpu.py -s
    python tools/action_decoder_margins_md.py margins.jsonl profiles/action_decoder_module_margins.md

(one JSON line per comparison, tests/golden_util.record_margin).  Run it where the tests ran: the header names that box."""
import collections
import json
import socket
import sys

import torch

rows = [json.loads(l) for l in open(sys.argv[1])]
rows = [r for r in rows if 'test_action_decoder_gpu' in r['test']]
OUT = sys.argv[2]
box = socket.gethostname()
if torch.cuda.is_available():
    p = torch.cuda.get_device_properties(0)
    box += f", {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"
out = []
out.append("# Action decoder as a module: measured margins\n")
out.append("Formatted by `tools/action_decoder_margins_md.py` from the margins one run of `tests/test_action_decoder_gpu.py` recorded\n"
           "(`golden_util.record_margin`).  Measured on: " + box + ".\n"
           "The fp64 / bf16-rounded references and the floors are CPU evaluations of `tests/action_decoder_util.py` on that box's host.\n"
           "Case tags: B / Tm / H / K = P + E / L.\n")
out.append("## f32 against fp64: tolerance-use\n")
out.append("`|got - ref64| / (1e-4 (|ref| + median|ref|) + 4 |ref32 - ref64|)`, worst element; 1.0 is the bound.  `grads`: the worst over\nall parameter gradients, with its name.\n")
f = [r for r in rows if r['kind'] == 'f32 tolerance-use' and r['tensor'].startswith('f32 B')]
cases = collections.OrderedDict()
for r in f:
    tag, q = r['tensor'].rsplit(' ', 1)
    cases.setdefault(tag[4:], {})[q] = r['err']
out.append("| case | loss | heads | hidden states (per layer) | dx_seq | grads (worst) |")
out.append("|---|---|---|---|---|---|")
for c, d in cases.items():
    hs = ", ".join("%.2g" % d[k] for k in sorted(d) if k[0] == 'h' and k[1:].isdigit())
    g = {k: v for k, v in d.items() if '.' in k}
    gw = max(g, key=g.get)
    out.append(f"| {c} | {d['loss']:.2g} | {d['heads']:.2g} | {hs} | {d['dx_seq']:.2g} | {g[gw]:.2g} (`{gw}`) |")
k = [r for r in rows if r['kind'] == 'f32 tolerance-use' and not r['tensor'].startswith('f32 B')]
groups = collections.OrderedDict()
for r in k:
    name = r['tensor'].split(' ')[0]
    groups[name] = max(groups.get(name, 0.0), r['err'])
out.append("\nKernel-level f32 rule (`rtol` 1e-5 over the sums of the products' magnitudes), worst tolerance-use over all cases of a test:\n")
out.append("| test | worst |")
out.append("|---|---|")
for n, v in groups.items():
    out.append(f"| {n} | {v:.2g} |")
out.append("\n## bf16 against the restatement with bf16 operand rounding\n")
out.append("Relative norms.  bound = max(project constant, 3 x floor): 2e-3 for loss / heads / hidden states, 1e-2 for gradients\n"
           "(`tests/test_kernels_gpu.py`); floor = the rounded restatement re-evaluated under 1-ulp weight perturbations\n"
           "(`golden_util.gradient_floor`).  Per case the worst forward quantity and the worst gradient by err / bound, and every quantity\nwhose bound came from the floor.\n")
b = [r for r in rows if r['kind'] == 'bf16 vs rounded restatement']
cases = collections.OrderedDict()
for r in b:
    tag, q = r['tensor'].rsplit(' ', 1)
    cases.setdefault(tag, []).append((q, r['err'], r['floor'], r['tol']))
isf = lambda q: q in ('loss', 'heads') or (q[0] == 'h' and q[1:].isdigit())
out.append("| case | worst forward: err / floor / bound | worst gradient: err / floor / bound | bounds set by the floor |")
out.append("|---|---|---|---|")
for c, L in cases.items():
    wf = max((x for x in L if isf(x[0])), key=lambda x: x[1] / x[3])
    wg = max((x for x in L if not isf(x[0])), key=lambda x: x[1] / x[3])
    fl = [f"`{q}` {t:.2g}" for q, e, f_, t in L if t > (2e-3 if isf(q) else 1e-2) * 1.0000001]
    fmt = lambda x: f"`{x[0]}` {x[1]:.2g} / {x[2]:.2g} / {x[3]:.2g}"
    out.append(f"| {c} | {fmt(wf)} | {fmt(wg)} | {', '.join(fl) if fl else '-'} |")
out.append("\n## bf16: ReLU decisions that differ from the restatement's away from a tie\n")
out.append("Share of a layer's gates (and their number).  `own`: the rounded restatement against itself under the floor's 1-ulp weight\n"
           "perturbations, the worst of the runs; the module may differ in at most 3 x as many.  Cases that are not listed: none on either side.\n")
out.append("| case | layer | module | restatement's own | cap |")
out.append("|---|---|---|---|---|")
for r in rows:
    if r['kind'] == 'bf16 gate disagreement' and (r['err'] > 0 or r['floor'] > 0):
        tag, l = r['tensor'].rsplit(' layer ', 1)
        B_, Tm_, H_ = (int(x[len(k):]) for x, k in zip(tag.split('/')[:3], ('B', 'Tm', 'H')))
        n = B_ * Tm_ * H_
        out.append(f"| {tag} | {l} | {r['err']:.2g} ({round(r['err'] * n)}) | {r['floor']:.2g} ({round(r['floor'] * n)}) | {r['tol']:.2g} |")
out.append("\n## Route against route and the twin pass (bf16, same operands)\n")
out.append("bound = max(2e-5, 3 x floor) on relative norms; the worst quantity per variant by err / bound.  Every bound above 2e-5 is set by the floor:\n"
           "the floor of a gradient through Tm rounded ReLU-RNN steps is 1e-4 .. 2e-2, so for these quantities the comparison\nis only as sharp as the reference's own reproducibility; what the routes actually differ by is the `err` column.\n")
p = [r for r in rows if r['kind'] == 'route vs route']
cases = collections.OrderedDict()
for r in p:
    tag, q = r['tensor'].rsplit(' ', 1)
    cases.setdefault(tag, []).append((q, r['err'], r['floor'], r['tol']))
out.append("| variant | worst: err / floor / bound | largest err of any quantity |")
out.append("|---|---|---|")
for c, L in cases.items():
    w = max(L, key=lambda x: x[1] / x[3])
    m = max(L, key=lambda x: x[1])
    out.append(f"| {c} | `{w[0]}` {w[1]:.2g} / {w[2]:.2g} / {w[3]:.2g} | `{m[0]}` {m[1]:.2g} |")

# ---- appendix: every quantity
out.append("")
out.append("## Appendix: every quantity\n")
out.append("### f32 tolerance-use\n")
f = [r for r in rows if r['kind'] == 'f32 tolerance-use' and r['tensor'].startswith('f32 B')]
cases = collections.OrderedDict()
for r in f:
    tag, q = r['tensor'].rsplit(' ', 1)
    cases.setdefault(tag[4:], collections.OrderedDict())[q] = r['err']
qs = []
for d in cases.values():
    for q in d:
        if q not in qs:
            qs.append(q)
out.append("| quantity | " + " | ".join(cases) + " |")
out.append("|---|" + "---|" * len(cases))
for q in qs:
    out.append(f"| `{q}` | " + " | ".join(("%.2g" % d[q]) if q in d else "" for d in cases.values()) + " |")
out.append("\n### bf16: err / floor / bound (`*`: the bound is 3 x floor)\n")
b = [r for r in rows if r['kind'] == 'bf16 vs rounded restatement']
cases = collections.OrderedDict()
for r in b:
    tag, q = r['tensor'].rsplit(' ', 1)
    cases.setdefault(tag, collections.OrderedDict())[q] = r
for c, d in cases.items():
    out.append(f"**{c}**: " + "; ".join(
        f"`{q}` {r['err']:.2g} / {r['floor']:.2g} / {r['tol']:.2g}" + ("*" if r['tol'] > (2e-3 if isf(q) else 1e-2) * 1.0000001 else "")
        for q, r in d.items()) + "\n")
open(OUT, 'w').write("\n".join(out) + "\n")
