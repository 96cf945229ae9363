"""Time the relay-imitation rollout step for R environments on one GPU (profiles/ril_rollout.md): the configured module
(config/module/relay_imitation_learning.yaml: two 4 x 1024 SiLU policies, a 64 -> 256 -> 256 -> 32 goal encoder, two cameras) at
R in {1, 8, 9, 16, 24, 32, 64}:

  - the low-level chain [state | sub-goal] -> action forced through each route of RelayPolicy - "rows": ONE
    tacorl_rows_mlp_fwd call; "composed": ops.mlp_fwd + ops.tanh_normal_sample, kernels that predate the rows chain - and
    as the policy routes it itself;
  - the high-level re-plan (goal encoder + high-level chain) the same three ways;
  - RelayPolicy.step_embeddings, decoding and re-planning, as it routes itself;
  - the rows route of the low-level chain with one and with two neurons per wave in the hidden layers (bit-identical
    results: tests/test_rows_policy_gpu.py).

    python tools/time_ril_rollout.py [--steps 200] [--warmup 20] [--out profiles/ril_rollout.md]

All arms run in the same process, interleaved step by step in a shuffled order on the same weights and inputs; HIP events
around every call, the median of --steps after --warmup; every call queued behind a spin kernel (the device's time for the
arm), then once more from an idle GPU (`interleaved`).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (1, 8, 9, 16, 24, 32, 64)
SPREAD = 1.03   # the box-to-box spread of README.md: routed <= the faster forced arm x 1.03
NPW_GAIN = 1.03  # one neuron per wave is kept only where it is faster by more than this at R = 1 and R = 8


SPIN_TICKS = 40000  # 400 us of the device's 100 MHz clock: longer than the host needs to queue any arm


def interleaved(fns, steps, warmup, spin=None):
    """{name: median us}: the callables take turns, one call each per round, the order shuffled per round.  Every call starts from the
    same state of the stream - otherwise its time depends on the arm before it (behind a long arm the host has queued the whole
    chain before the first event is reached and the launch latency is hidden, behind a short one it is not: identical arms
    then differ by 20 %).  spin: a callable that queues a spin kernel (tacorl_time_spin) behind the synchronisation - the arm is
    then queued while the GPU is busy, as a policy step is behind the encoders, and the bracket holds the device's time for it;
    None: from an idle GPU, the bracket holds the host's launch path too."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    names, rng = list(fns), random.Random(0)
    for _ in range(steps):
        rng.shuffle(names)  # (a fixed order gives every arm one predecessor, whose leavings in the caches it then inherits)
        for k in names:
            f = fns[k]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            if spin is not None:
                spin()
            a.record()
            f()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    med = lambda ts: sorted(ts)[len(ts) // 2] * 1e3  # noqa: E731
    return {k: med([a.elapsed_time(b) for a, b in v]) for k, v in evs.items()}


def build(dev):
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning
    from tests import ril_util as U

    torch.manual_seed(0)
    mod = RelayImitationLearning(device=dev, **U.ril_cfg(low=["rgb_static", "rgb_gripper"], high=["rgb_gripper", "rgb_static"]))
    mod.eval()
    return mod


def case(mod, R, dev, steps, warmup):
    from tacorl_amd import ops
    from tacorl_amd._lib import call, ptr
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    pol = RelayPolicy(mod, n_envs=R, plan_duration=1 << 30)
    g = torch.Generator().manual_seed(R)
    obs = {c: torch.randn(R, 32, generator=g).to(dev) for c in pol.cams}
    goal = {c: torch.randn(R, 32, generator=g).to(dev) for c in pol.cams}
    pol.reset()
    pol.step_embeddings(obs, goal)
    low = lambda npw: (lambda: pol.low.run(pol.lin, pol.ld, R, pol.actions, 0, pol.A, "rows", npw=npw))  # noqa: E731

    def replan_step():
        pol.reset()
        pol.step_embeddings(obs, goal)

    arms = {
        "low_rows": lambda: pol.decode(obs, route="rows"), "low_composed": lambda: pol.decode(obs, route="composed"),
        "low_routed": lambda: pol.decode(obs),
        "replan_rows": lambda: pol.replan(obs, goal, R, route="rows"), "replan_composed": lambda: pol.replan(obs, goal, R, route="composed"),
        "replan_routed": lambda: pol.replan(obs, goal, R),
        "step_decode": lambda: pol.step_embeddings(obs, goal), "step_replan": replan_step,
        "npw1": low(1), "npw2": low(2)}
    marks = torch.zeros(2, dtype=torch.int64, device=dev)
    t = interleaved(arms, steps, warmup, spin=lambda: call("tacorl_time_spin", ptr(marks), 0, SPIN_TICKS, ops.stream()))
    idle = interleaved(arms, steps, warmup)
    r = {k: round(v, 2) for k, v in t.items()}
    r["idle"] = {k: round(v, 2) for k, v in idle.items()}
    r["route"] = pol.rows_route(R)
    r["auto_npw"] = ops.L.lib().tacorl_rows_mlp_npw(pol.low.dims[1], R)
    for k in ("low", "replan"):
        r[k + "_ratio"] = round(t[k + "_routed"] / min(t[k + "_rows"], t[k + "_composed"]), 3)
    return r


def markdown(out):
    rows = out["rows"]
    chain_mb = out["chain_bytes"] / 1e6
    L = ["# The relay-imitation rollout step", "",
         f"`tools/time_ril_rollout.py` on {out['device']}: two 4 x 1024 SiLU policies on [64 | 32] inputs ({chain_mb:.1f} MB of fp32 "
         f"weights per policy), fp32, HIP events, {out['warmup']} warm-up steps, the median of {out['steps']}; all arms interleaved in "
         f"one process in an order shuffled per round.  Every call is queued behind a synchronisation and a 400 us spin kernel, so the host has "
         f"queued the arm before the GPU reaches it - as a policy step is queued behind the encoders - and the bracket holds the "
         f"device's time; the last section repeats the arms from an idle GPU, where the bracket holds the host's launch path too.  `rows`: one `tacorl_rows_mlp_fwd` call per chain; `composed`: `ops.mlp_fwd` + `ops.tanh_normal_sample` on "
         "pre-allocated buffers - kernels that exist without the rows chain, the yardstick; `routed`: as `RelayPolicy.rows_route` "
         f"chooses (`rows` up to R = {out['max_r']}).  Times in microseconds.", "",
         "## The low-level chain (every step)", "",
         "| R | route | routed | rows | composed | routed / faster arm |", "|---|---|---|---|---|---|"]
    for R, r in rows.items():
        L.append(f"| {R} | {r['route']} | {r['low_routed']} | {r['low_rows']} | {r['low_composed']} | {r['low_ratio']} |")
    L += ["", "## The high-level re-plan (goal encoder + chain, all R rows due)", "",
          "| R | route | routed | rows | composed | routed / faster arm |", "|---|---|---|---|---|---|"]
    for R, r in rows.items():
        L.append(f"| {R} | {r['route']} | {r['replan_routed']} | {r['replan_rows']} | {r['replan_composed']} | {r['replan_ratio']} |")
    L += ["", "## RelayPolicy.step_embeddings", "", "| R | decoding step | re-planning step (every row due) |", "|---|---|---|"]
    for R, r in rows.items():
        L.append(f"| {R} | {r['step_decode']} | {r['step_replan']} |")
    L += ["", "## Neurons per wave in the hidden layers (low-level chain, rows route)", "",
          "| R | one neuron per wave | two neurons per wave | two / one | the library's choice (`npw = 0`) |", "|---|---|---|---|---|"]
    for R, r in rows.items():
        L.append(f"| {R} | {r['npw1']} | {r['npw2']} | {r['npw2'] / r['npw1']:.3f} | {r['auto_npw']} |")
    gain = {R: rows[R]["npw2"] / rows[R]["npw1"] for R in ("1", "8") if R in rows}
    keep = bool(gain) and all(v > NPW_GAIN for v in gain.values())
    wrong = [R for R, r in rows.items() if r["npw" + str(3 - r["auto_npw"])] * SPREAD < r["npw" + str(r["auto_npw"])]]
    L += ["", "Two neurons per wave give a 1024-wide layer 128 workgroups per group of 8 rows, half the GPU's 256 CUs.  The bar "
          "for choosing one neuron per wave: the low-level chain faster by more than 3 % at R = 1 AND at R = 8.  Measured two / one = "
          + ", ".join(f"{v:.3f} at R = {R}" for R, v in gain.items()) + f": the bar is {'met' if keep else 'NOT met'}.  "
          "The library's choice (`rows_mlp_auto_npw`, `csrc/rollout_ops.hip`) is the last column; `npw = 1 / 2` force an arm, and "
          "both give the same bits (`tests/test_rows_policy_gpu.py`).  The action decoder's `tacorl_rows_linear2_fwd` keeps two."
          + ("" if not wrong else "  The arm not chosen is faster by more than the 3 % spread at R = " + ", ".join(wrong) + ".")]
    bad = [(k, R, r[k + "_ratio"]) for R, r in rows.items() for k in ("low", "replan") if r[k + "_ratio"] > SPREAD]
    L += ["", "## The claim", "",
          "At every R measured the self-routed low-level chain and the self-routed re-plan take at most 1.03 x the faster forced arm: "
          + ("holds." if not bad else "does NOT hold at " + ", ".join(f"{k} R = {R} ({v} x)" for k, R, v in bad) + ".")]
    L += ["", "| R | low-level chain | re-plan |", "|---|---|---|"]
    for R, r in rows.items():
        ok = lambda v: "holds" if v <= SPREAD else "fails"  # noqa: E731
        L.append(f"| {R} | {ok(r['low_ratio'])} ({r['low_ratio']}) | {ok(r['replan_ratio'])} ({r['replan_ratio']}) |")
    faster = [R for R, r in rows.items() if r["low_rows"] <= r["low_composed"] and r["replan_rows"] <= r["replan_composed"]]
    L += ["", f"`RelayPolicy.ROWS_KERNEL_MAX_R` = {out['max_r']}.  The rows route is the faster arm of both chains at R in "
          f"[{', '.join(faster)}] of [{', '.join(rows)}]: the composed arm sends at most 64 rows through the training GEMMs' "
          "tiles, one launch per layer and one for the sampler; the rows chain reads the weights once more per further group of 8 rows.  "
          "The threshold started at 16, the action decoder's value, and was set from this table."]
    L += ["", "## From an idle GPU", "",
          "The same arms with nothing queued in front of them (a synchronisation, no spin kernel): the bracket starts when the host "
          "starts to launch, so it holds the host's launch path as well - what a caller pays who has nothing else queued.", "",
          "| R | low routed | low rows | low composed | re-plan routed | re-plan rows | re-plan composed | decoding step | re-planning step | "
          "one neuron per wave | two |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for R, r in rows.items():
        i = r["idle"]
        L.append(f"| {R} | {i['low_routed']} | {i['low_rows']} | {i['low_composed']} | {i['replan_routed']} | {i['replan_rows']} | "
                 f"{i['replan_composed']} | {i['step_decode']} | {i['step_replan']} | {i['npw1']} | {i['npw2']} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ril_rollout.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ril_rollout: needs a GPU")
    from tacorl_amd import _lib, blocks
    from tacorl_amd.evaluation.vec_policy import RelayPolicy

    dev = "cuda:0"
    _lib.call("tacorl_hip_init", 0)
    mod = build(dev)
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "max_r": RelayPolicy.ROWS_KERNEL_MAX_R,
           "chain_bytes": 4 * blocks.mlp_size(mod.engine.pol_dims["low"]), "rows": {}}
    for R in ROWS:
        out["rows"][str(R)] = case(mod, R, dev, a.steps, a.warmup)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(out))


if __name__ == "__main__":
    main()
