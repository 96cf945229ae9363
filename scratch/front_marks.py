"""The front as the step pays it (profiles/step_front.md section 1): the per-step period of the headline step - HIP events
over bursts of 200 graph replays, one batch as in bench.py - minus the front:start -> step:end span of each burst's last
replay (device marks, ops.trace_marks).  First unmarked (the marks' own cost), then marked.  Prints one "FRONT {json}" line."""
import os, sys, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch, bench
from tacorl_amd import _lib, ops
dev = torch.device("cuda:0"); _lib.call("tacorl_hip_init", 0)
res = {}
for traced in (False, True):
    reader = ops.trace_marks(dev) if traced else None
    mod = bench.build_module(dev, "bf16", 16, 1)
    batch = bench.synth_batch(256, 16, 84, 84, dev, 1)  # (bench.py reuses one batch)
    mod.enable_graph(); mod.log_every_n_steps = 50
    def run(n):
        for i in range(n): mod.training_step(batch, i)
    run(20); torch.cuda.synchronize()
    per, spans, fronts = [], [], []
    for burst in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(200); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 200
        per.append(ms)
        if traced:
            m = dict(reader())
            span = m["step:end"] - m["front:start"]
            spans.append(span); fronts.append(ms * 1000 - span)
    key = "traced" if traced else "untraced"
    res[key + "_ms_per_step"] = [round(x, 4) for x in per]
    if traced:
        res["span_us"] = [round(x, 1) for x in spans]
        res["front_us"] = [round(x, 1) for x in fronts]
        res["last_marks"] = [(n, round(t, 1)) for n, t in reader()]
print("FRONT " + json.dumps(res), flush=True)
