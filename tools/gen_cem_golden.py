"""Generate the CEM refinement fixtures tests/golden/cem_cql.npz and tests/golden/cem_tacorl.npz by driving the UNMODIFIED
reference CEMOptimizer (modules/cem/cem.py) on CPU, on unbatched observations (the only form it runs on: images (3,H,W)).

Build container only (needs the reference tree, like oracle/gen_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_cem_golden.py            # both files
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_cem_golden.py cem_cql

Nothing under oracle/ changes; its harness is imported.  A file holds, as every fixture here, the seeds from which
tacorl_amd.synth re-derives the module's parameters and the images, plus per case: the CEM parameters, the standard-normal
draws (`eps`, recovered by the harness's patched Normal.sample), the starting mean, and per iteration Q, elite indices,
mean and std the reference computed, and the action it returned.  The population is not stored: it is
clamp(mean + std * eps, -1, 1) of stored arrays (tests/cem_util.py derives it), and it does not compress.  The two critics' embeddings of the
observation are stored too, so that a CPU test can restate the refinement without an encoder.

Q forms: 'as written' hands the reference its own q1 and q2 (it evaluates q1 twice); 'twin' hands it q1 := min(q1, q2) as a
callable - the class itself is the reference's in both.

The critics' output layers are scaled by `out_scale`, so that the spread of Q over a population is comparable to |Q|.
Elite selection is discontinuous, so a case is re-seeded until, in every iteration, both the gap between the n_elite-th and
the (n_elite+1)-th Q value and the gap between the best and the second best are >= GAP * max|Q| of that iteration; the seed
and the smallest relative gap are stored, and tests/test_cem_cpu.py asserts the gap on load.  The ORDER of the elites is
compared too, wherever two neighbouring elites are at least ORDER_GAP * max|Q| apart (the fp32 tolerance itself: closer ones
may legitimately swap, and requiring every neighbouring pair of 26 elites in 4 iterations to be that far apart rejects nearly
every seed); the margin and each case's smallest neighbouring gap are stored for the tests.

The reference runs in fp64 (module.double(), fp64 default dtype): its code is the same, and the fixture then carries none of
its own fp32 rounding - in fp32 its Q values sit up to 1.5e-6 (relative l2, measured) from their fp64 values, more than the
1e-6 the CPU test allows the restatement.  Arrays are stored as fp32 (the embeddings and the actor's mean as fp64); the
stored `eps` is the fp32 rounding of the draws, what every consumer of the fixture is given.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as H  # noqa: E402
from tacorl_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
GAP = 1e-3
ORDER_GAP = 1e-4
FILES = {
    "cem_cql": dict(kind="cem_cql", cams={"rgb_static": (84, 84)}, seed=61, out_scale=8.0, discrete_gripper=True),
    "cem_tacorl": dict(kind="cem_tacorl", cams={"rgb_static": (84, 84)}, latent=16, seed=62, out_scale=8.0,
                       discrete_gripper=False),
}
# (name, batch_size, initial_mean from the actor?, twin minimum?): both population sizes, both starting means and both Q
# forms in each file; the A = 16 file leaves out the two N = 64 cases whose (mean, Q form) its N = 256 cases already hold
ALL = [("n64_actor", 64, True, False), ("n64_actor_twin", 64, True, True), ("n64_zero", 64, False, False),
       ("n64_zero_twin", 64, False, True), ("n256_actor", 256, True, False), ("n256_zero_twin", 256, False, True)]
CASES = {"cem_cql": ALL, "cem_tacorl": [c for c in ALL if c[0] not in ("n64_actor", "n64_zero_twin")]}


def rel_gaps(q, n_elite):
    """(elite-boundary gap, best gap) of one iteration's Q values, relative to max|Q|."""
    s = np.sort(np.asarray(q, dtype=np.float64))[::-1]
    m = np.abs(s).max()
    return (s[n_elite - 1] - s[n_elite]) / m, (s[0] - s[1]) / m


def order_gap(q, n_elite):
    """Smallest gap between two neighbouring elites of one iteration, relative to max|Q|."""
    s = np.sort(np.asarray(q, dtype=np.float64))[::-1]
    return float(np.min(s[: n_elite - 1] - s[1:n_elite]) / np.abs(s).max())


def run_one(mod, obs, mean0, N, twin, dg, A, eps_seed):
    from tacorl.modules.cem.cem import CEMOptimizer

    rec = dict(pop=[], q=[], elite=[], mean=[], std=[])
    calls = [0]

    def q_rec(o, actions):
        v = torch.min(mod.q1(o, actions), mod.q2(o, actions)) if twin else mod.q1(o, actions)
        if calls[0] % 2 == 0:  # the reference evaluates its q1 twice per iteration
            rec["pop"].append(actions.clone())
            rec["q"].append(v.reshape(-1).clone())
        calls[0] += 1
        return v

    cem = CEMOptimizer(q1=q_rec, q2=mod.q2, batch_size=N, action_dim=A, discrete_gripper=dg)
    upd = cem.update_population_parameters

    def upd_rec(elites, mean, std):
        m, s = upd(elites=elites, mean=mean, std=std)
        rec["mean"].append(m.clone())
        rec["std"].append(s.clone())
        return m, s

    cem.update_population_parameters = upd_rec
    o_argsort = torch.argsort

    def argsort_rec(*a, **k):
        r = o_argsort(*a, **k)
        rec["elite"].append(r[: int(np.round(N * cem.elite_fraction)), 0].clone())
        return r

    tape = H.NoiseTape()
    torch.manual_seed(eps_seed)
    torch.argsort = argsort_rec
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad(), H.record_noise(tape):
            action = cem.get_action(obs, initial_mean=mean0)
    finally:
        torch.argsort = o_argsort
        torch.set_default_dtype(torch.float32)
    eps = torch.stack(tape.of_kind("normal"))
    assert eps.shape == (cem.num_iterations, N, A) and len(rec["q"]) == cem.num_iterations
    hp = dict(batch_size=N, num_iterations=cem.num_iterations, elite_fraction=cem.elite_fraction, min_std=cem.min_std,
              max_std=cem.max_std, alpha=cem.alpha, action_dim=A, discrete_gripper=bool(dg), twin_min=bool(twin))
    return action, eps, {k: torch.stack(v) for k, v in rec.items()}, hp


def run_file(name, c):
    torch.manual_seed(c["seed"])
    torch.set_num_threads(8)
    cams, dg = c["cams"], c["discrete_gripper"]
    names = tuple(sorted(cams))
    if c["kind"] == "cem_tacorl":
        mod = H.build_tacorl(H.build_play_lmp(cams=names, latent_plan_dim=c["latent"], seq_len=16), finetune_action_decoder=False)
        A = c["latent"]
    else:
        mod = H.build_cql(cams=names)
        A = 7
    synth.fill_params_(mod, c["seed"])
    with torch.no_grad():
        for q in (mod.q1, mod.q2):
            q.critic.Q.out.weight.mul_(c["out_scale"])
            q.critic.Q.out.bias.mul_(c["out_scale"])
    mod.double().eval()
    if c["kind"] == "cem_tacorl":
        b = synth.make_play_batch(c["seed"] * 100, 1, 2, cams)
        obs1 = {"observation": {k: v[:, 0] for k, v in b["states"].items()}, "goal": b["goal"]}
    else:
        obs1 = synth.make_transition_batch(c["seed"] * 100, 1, cams)["observations"]
    obs1 = {k: {cam: v.double() for cam, v in d.items()} for k, d in obs1.items()}
    obs = {k: {cam: v[0] for cam, v in d.items()} for k, d in obs1.items()}  # unbatched (3,H,W)
    out = {}
    with torch.no_grad():
        actor_mean = mod.actor.get_actions(obs1, deterministic=True, reparameterize=False)[0].reshape(-1).clone()  # (one row: the encoder squeezes)
        out["emb_q1"] = mod.q1.get_emb_representation(obs1).reshape(-1).numpy()
        out["emb_q2"] = mod.q2.get_emb_representation(obs1).reshape(-1).numpy()
    out["actor_mean"] = actor_mean.numpy()
    assert actor_mean.shape == (A,) and out["emb_q1"].ndim == 1
    meta = []
    for cname, N, from_actor, twin in CASES[name]:
        ci = [a[0] for a in ALL].index(cname)
        n_elite = int(np.round(N * 0.1))
        for attempt in range(400):
            eps_seed = c["seed"] * 100000 + ci * 4000 + attempt
            action, eps, rec, hp = run_one(mod, obs, actor_mean if from_actor else None, N, twin, dg, A, eps_seed)
            gaps = [g for q in rec["q"] for g in rel_gaps(q.numpy().astype(np.float32), n_elite)]
            ogap = min(order_gap(q.numpy().astype(np.float32), n_elite) for q in rec["q"])
            if min(gaps) >= GAP:
                break
        else:
            raise RuntimeError(f"{name}/{cname}: no seed met the gap condition")
        q = rec["q"].numpy()
        print(f"[{name}/{cname}] seed {eps_seed} (attempt {attempt}), min rel gap {min(gaps):.3g}, order gap {ogap:.3g}, per-iteration Q spread / "
              f"max|Q|: {[round(float(x.std() / np.abs(x).max()), 3) for x in q]}, action {action.numpy().round(3)}")
        pre = f"c/{cname}/"
        out[pre + "eps"] = eps.numpy().astype(np.float32)
        out[pre + "q"] = q.astype(np.float32)
        out[pre + "elite"] = rec["elite"].numpy().astype(np.int32)
        out[pre + "mean"] = rec["mean"].numpy().astype(np.float32)
        out[pre + "std"] = rec["std"].numpy().astype(np.float32)
        out[pre + "action"] = action.numpy().astype(np.float32)
        meta.append(dict(name=cname, from_actor=from_actor, eps_seed=eps_seed, min_rel_gap=float(min(gaps)), min_order_gap=float(ogap), **hp))
    out["param_names"] = np.array([n for n, _ in mod.named_parameters()])
    out["param_shapes"] = np.array(json.dumps([list(p.shape) for _, p in mod.named_parameters()]))
    out["param_requires_grad"] = np.array([p.requires_grad for _, p in mod.named_parameters()])
    out["config"] = np.array(json.dumps(dict(c, B=1, T=2, gap=GAP, order_gap=ORDER_GAP, cases=meta)))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(FILES):
        run_file(n, FILES[n])
