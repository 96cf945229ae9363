"""Measure the two things the long-horizon rollout evaluation changes, on one MI355X, and write profiles/rollout_lh.md.

    python tools/time_rollout_lh.py [--out profiles/rollout_lh.md]

1. A step's draws: utils/callbacks/rollout.py RolloutBase._noise (2 R hashed host generators per step, up to 2 R more on a
   re-planning step, stacked and uploaded) against ONE noise.py RowNoise.fill (utils/callbacks/rollout_long_horizon.py
   row_noise), at R = 16 and 64, with and without a CEM segment; the decoder's and CEM's default sizes (Da 7, K 10, P 16;
   4 iterations of 256 candidates); plan_duration 16.  Per step two host clocks: until the call returns ("host") and until
   the draws are on the device (a synchronise behind it: "ready").  The two paths alternate step by step; median over 200
   steps after 20 of warm-up, and the median over the re-planning steps among them alone.
2. Policy calls per evaluation: 32 scripted episodes (lengths 20 .. 300, seeded) over R = 8 through rollout_episodes_refill
   with refill=True and refill=False and a policy that does nothing.  Counted, not timed.

It needs a GPU for part 1 and refuses to run without one."""
import argparse
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tacorl_amd.evaluation.vec_policy import PlanClock, rollout_episodes_refill  # noqa: E402
from tacorl_amd.utils.callbacks.rollout import RolloutBase  # noqa: E402
from tacorl_amd.utils.callbacks.rollout_long_horizon import row_noise  # noqa: E402
from tests import rollout_lh_envs as LH  # noqa: E402

DEV, DUR, STEPS, WARM = "cuda:0", 16, 200, 20


def _pol(R, cem):
    return NS(R=R, dev=DEV, plan_duration=DUR, actor=None, ad=NS(Da=7, K=10, P=16),
              cem=NS(num_iterations=4, batch_size=256, action_dim=16) if cem else None)


def time_draws(R, cem):
    pol, keys = _pol(R, cem), list(range(R))
    host_at = RolloutBase._noise(NS(seed=0), pol, keys)
    dev_at = row_noise(pol, 0)
    t = {k: [] for k in ("host/host", "host/ready", "device/host", "device/ready")}
    replan = []
    for s in range(-WARM, STEPS):
        step = s % (4 * DUR)
        due = keys if step % DUR == 0 else []
        for name in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host":
                out = {k: v.to(DEV) for k, v in host_at(step).items()}  # what policy.step does with a host tensor
            else:
                out = dev_at(keys, [step] * R, due)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert out
            if s >= 0:
                t[f"{name}/host"].append(t1 - t0)
                t[f"{name}/ready"].append(t2 - t0)
        if s >= 0:
            replan.append(bool(due))
    replan = np.array(replan)
    med = {k: (1e6 * float(np.median(v)), 1e6 * float(np.median(np.array(v)[replan]))) for k, v in t.items()}
    return med, int(replan.sum())


class _Idle:
    """A policy of R rows that does nothing: its calls are counted."""

    def __init__(self, R):
        self.R, self.clock, self.calls = R, PlanClock(R, DUR), 0

    def reset(self, rows=None):
        self.clock.reset(rows)

    def step(self, observation, goal, noise=None):
        self.calls += 1
        self.clock.tick(set(self.clock.due()))
        return torch.zeros(self.R, 8)


def count_calls(R=8, n=32, seed=0):
    lengths = np.random.RandomState(seed).randint(20, 301, size=n).tolist()
    episodes = [(i, {"length": m, "seed": i}) for i, m in enumerate(lengths)]
    calls = {}
    for refill in (True, False):
        pol = _Idle(R)
        infos = rollout_episodes_refill(pol, [LH.ScriptedVectorEnv(max_episode_steps=300) for _ in range(R)], episodes, refill=refill)
        assert [i["episode_length"] for i in infos] == lengths
        calls[refill] = pol.calls
    assert calls[True] == LH.greedy_makespan(lengths, R) and calls[False] == LH.batch_makespan(lengths, R)
    return lengths, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_lh.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_rollout_lh.py times device work: it needs a GPU")
    rows = []
    for R in (16, 64):
        for cem in (False, True):
            med, n_replan = time_draws(R, cem)
            rows.append((R, cem, med, n_replan))
            print(R, cem, med, flush=True)
    lengths, calls = count_calls()
    L = ["# Long-horizon rollout evaluation: a step's draws and the policy calls of an evaluation", "",
         f"`python tools/time_rollout_lh.py` on one MI355X ({torch.cuda.get_device_name(0)}), torch {torch.__version__}.", "",
         "## A step's draws", "",
         "`RolloutBase._noise` (hashed host generators, stacked, uploaded with `.to(device)`) against one `RowNoise.fill`",
         f"(`tacorl_noise_fill_rows`): Da 7, K 10, P 16, CEM 4 x 256 x 16 per row, plan_duration {DUR}.  Microseconds of host clock per",
         f"step, median over {STEPS} steps after {WARM} of warm-up, the two paths alternating; in brackets the median over the",
         "re-planning steps among them.  host: until the call returns; ready: until a synchronise behind it returns.", "",
         "| R | CEM | generators: host | generators: ready | one fill: host | one fill: ready |", "|---|---|---|---|---|---|"]
    f = lambda m: f"{m[0]:.0f} ({m[1]:.0f})"  # noqa: E731
    for R, cem, med, n_replan in rows:
        L.append(f"| {R} | {'yes' if cem else 'no'} | {f(med['host/host'])} | {f(med['host/ready'])} | {f(med['device/host'])} | "
                 f"{f(med['device/ready'])} |")
    L += ["", f"({rows[0][3]} of the {STEPS} steps re-plan.)", "", "## Policy calls per evaluation", "",
          f"32 scripted episodes, lengths drawn uniformly from 20 .. 300 (seed 0; sum {sum(lengths)}, longest {max(lengths)}), over R = 8",
          "slots, counted with a policy that does nothing:", "",
          "| runner | policy calls |", "|---|---|", f"| `refill=True` | {calls[True]} |", f"| `refill=False` (fixed batches of 8) | {calls[False]} |",
          f"| lower bound, ceil(sum / 8) | {-(-sum(lengths) // 8)} |", ""]
    with open(args.out, "w") as fh:
        fh.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
