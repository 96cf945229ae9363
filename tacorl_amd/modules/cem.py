"""Cross-entropy-method refinement of the actor's action (CQL) or latent plan (TACORL) against the critics - the
`use_cem` switch of the reference's rollout managers (reference modules/cem/cem.py; evaluation/rollout_manager.py:99-136,
:331-369):

    cem = CEMOptimizer(q1=module.q1, q2=module.q2, action_dim=module.actor.action_dim,
                       discrete_gripper=module.actor.discrete_gripper)
    initial_mean, _ = module.actor.get_actions(obs, deterministic=True, reparameterize=False)
    action = cem.get_action(obs, initial_mean=initial_mean).cpu().numpy()

The observation is encoded once per critic; the iterations - sample, evaluate, select, refit - are one HIP launch
(csrc/cem_ops.hip), one workgroup per observation row.  `cem_restatement` states the same algorithm in plain torch ops for
any device and dtype: the yardstick of the tests and the timing baseline of scratch/bench_cem.py.
"""
import numpy as np
import torch

from .. import ops
from .._lib import BF16, call
from .inference import CriticSurface


def n_elite_of(batch_size, elite_fraction):
    return int(np.round(batch_size * elite_fraction))


def cem_restatement(q_fn, emb, initial_mean, eps, *, n_elite, min_std=1e-3, max_std=0.3, alpha=0.1, discrete_gripper=False,
                    host_sync=False):
    """The reference's get_action for ONE observation on embeddings, in torch ops.
    q_fn(emb, actions (N,A)) -> (N,) or (N,1) Q values (whatever the caller wants maximised: q1, or min(q1, q2));
    emb: passed through to q_fn; initial_mean: (A,) or None; eps: (iters, N, A) standard-normal draws.
    host_sync: read the iteration's best Q back with .item() as the reference does (the timing baseline); otherwise the
    comparison stays on the device.  Returns (action (A,), trace) with trace = per-iteration lists 'pop', 'q', 'elite',
    'mean', 'std'."""
    iters, N, A = eps.shape
    mean = initial_mean.to(eps) if initial_mean is not None else torch.zeros(A, dtype=eps.dtype, device=eps.device)
    std = torch.ones(A, dtype=eps.dtype, device=eps.device) * max_std
    best_q, best_action = -float("inf"), None
    trace = dict(pop=[], q=[], elite=[], mean=[], std=[])
    for it in range(iters):
        actions = (mean + eps[it] * std).clamp(min=-1.0, max=1.0)
        if discrete_gripper:
            actions[..., -1] = torch.where(actions[..., -1] >= 0, 1.0, -1.0).to(actions)
        q = q_fn(emb, actions).reshape(N)
        elite = torch.argsort(q, dim=0, descending=True)[:n_elite]
        elites = actions[elite]
        mean = alpha * mean + (1 - alpha) * torch.mean(elites, dim=0)
        std = (alpha * std + (1 - alpha) * torch.std(elites, dim=0)).clamp(min=min_std, max=max_std)
        if host_sync:
            it_best = q[elite[0]].item()
            if it_best > best_q:
                best_q, best_action = it_best, elites[0]
        else:
            it_best = q[elite[0]]
            if best_action is None:
                best_q, best_action = it_best, elites[0]
            else:
                better = it_best > best_q
                best_q, best_action = torch.where(better, it_best, best_q), torch.where(better, elites[0], best_action)
        for k, v in (("pop", actions), ("q", q), ("elite", elite), ("mean", mean), ("std", std)):
            trace[k].append(v)
    return best_action, trace


class CEMOptimizer:
    """The reference's CEMOptimizer (constructor and get_action) on this project's critic surfaces.

    twin_min: the reference evaluates q1 twice and takes the minimum of the two equal values (cem.py:92-94), i.e. it maximises
    q1 alone; the default (False) executes exactly that.  twin_min=True maximises min(q1, q2), what the code reads as."""

    def __init__(self, q1, q2, batch_size=256, num_iterations=4, elite_fraction=0.1, min_std=1e-3, max_std=0.3, alpha=0.1,
                 action_dim=7, discrete_gripper=False, twin_min=False):
        surf = []
        for name, q in (("q1", q1), ("q2", q2)):
            cs = q if isinstance(q, CriticSurface) else getattr(q, "__dict__", {}).get("critic_surface")
            if not isinstance(cs, CriticSurface):
                raise TypeError(f"{name} must be a critic of a tacorl_amd module (module.q1 / q2 / target_q1 / target_q2), got "
                                f"{type(q).__name__}")
            surf.append(cs)
        self.q1, self.q2 = q1, q2
        self._s1, self._s2 = surf
        self.batch_size, self.num_iterations, self.elite_fraction = int(batch_size), int(num_iterations), elite_fraction
        self.min_std, self.max_std, self.alpha = float(min_std), float(max_std), float(alpha)
        self.action_dim, self.discrete_gripper, self.twin_min = int(action_dim), bool(discrete_gripper), bool(twin_min)
        self.n_elite = n_elite_of(self.batch_size, elite_fraction)
        if self.n_elite < 2:
            raise ValueError(f"batch_size {batch_size} * elite_fraction {elite_fraction} gives {self.n_elite} elite(s): the "
                             "unbiased std over fewer than 2 elites is NaN")
        if self.n_elite > self.batch_size or self.num_iterations < 1:
            raise ValueError(f"n_elite {self.n_elite} of {self.batch_size}, {self.num_iterations} iterations")
        if not (0.0 < self.min_std <= self.max_std) or not (0.0 <= self.alpha <= 1.0):
            raise ValueError(f"need 0 < min_std <= max_std and 0 <= alpha <= 1, got {min_std}, {max_std}, {alpha}")
        s1, s2 = surf
        if s1.owner is not s2.owner or (s1.E, s1.hidden, s1.q_layers) != (s2.E, s2.hidden, s2.q_layers):
            raise ValueError("q1 and q2 must be the twin critics of one module")
        if s1.A != self.action_dim:
            raise ValueError(f"action_dim {action_dim}: the critics take actions of {s1.A}")
        self.compute = s1.owner.compute
        if not ops.cem_supported(self.batch_size, self.action_dim, s1.E, s1.hidden, s1.q_layers, self.compute):
            raise NotImplementedError(
                f"fused CEM refinement: batch_size {self.batch_size} (a multiple of 64, at most 256), action_dim "
                f"{self.action_dim} (at most 32), embedding {s1.E} (at most 256), hidden {s1.hidden} (256), "
                f"{s1.q_layers} hidden Q layers (2 to 4) - outside the supported shapes")

    def _nets(self):
        return [self._s1, self._s2] if self.twin_min else [self._s1]

    def _mirrors(self, nets):
        """bf16 compute: the critics' bf16 weight mirrors, rewritten from the fp32 masters on every call (one launch of a few
        microseconds).  A version check is not enough here: the optimiser and Polyak kernels write the masters through raw
        pointers, so after a training step a mirror can be one step old while the tensor versions still agree."""
        if self.compute != BF16:
            return None
        blocks = [s.net for s in nets]
        call("tacorl_to_bf16_batch", len(blocks), ops.ptr_array([n.genc() for n in blocks]),
             ops.ptr_array([n.genc_bf16() for n in blocks]), (ops.C.c_long * len(blocks))(*[n.size - n.genc_off for n in blocks]),
             ops.stream())
        return [n.head_bf16() for n in blocks]

    @staticmethod
    def _unbatched(obs):
        if isinstance(obs, dict):
            return any(CEMOptimizer._unbatched(v) for v in obs.values())
        return obs.dim() in (1, 3)

    def get_action(self, obs, initial_mean=None, noise=None, return_trace=False):
        """obs: {'observation': {cam: img}, 'goal': {cam: img}} or an embedding, R >= 1 rows or unbatched; every row is an
        independent problem with its own draws.  initial_mean: (R,A), (A,) or None (zeros).  noise: {'eps': (R, iters, N, A)}
        injects the standard-normal draws.  Returns (R,A), or (A,) for an unbatched observation; with return_trace also a dict
        of per-iteration 'pop' (R,iters,N,A), 'q' (R,iters,N), 'elite' (R,iters,n_elite; descending Q), 'mean', 'std'
        (R,iters,A).  Everything is enqueued on the current stream; nothing is read back."""
        nets = self._nets()
        s1 = self._s1
        dev, A, N, iters = s1.owner.dev, self.action_dim, self.batch_size, self.num_iterations
        unbatched = self._unbatched(obs)
        if not isinstance(obs, dict) and len(nets) > 1:
            embs = [s1.emb_representation(obs)] * 2  # an embedding is taken as it is, by both critics
        else:
            embs = [s.emb_representation(obs) for s in nets]
        embs = [(e.unsqueeze(0) if e.dim() == 1 else e).contiguous() for e in embs]
        R = embs[0].shape[0]
        if embs[0].shape[1] != s1.E:
            raise ValueError(f"observation embedding has {embs[0].shape[1]} columns, the critics take {s1.E}")
        mean0 = None
        if initial_mean is not None:
            mean0 = initial_mean.to(dev, torch.float32).reshape(-1, A)
            if mean0.shape[0] != R:
                raise ValueError(f"initial_mean has {mean0.shape[0]} rows for {R} observation rows")
            mean0 = mean0.contiguous()
        if noise is not None:
            eps = noise["eps"].to(dev, torch.float32)
            if eps.numel() != R * iters * N * A:
                raise ValueError(f"noise['eps'] must be (R, iters, N, A) = {(R, iters, N, A)}, got {tuple(eps.shape)}")
            eps = eps.reshape(R, iters, N, A).contiguous()
        else:
            eps = torch.randn(R, iters, N, A, device=dev)
        out = torch.empty(R, A, device=dev)
        trace = None
        if return_trace:
            f = lambda *sh: torch.zeros(*sh, device=dev)  # noqa: E731
            trace = (f(R, iters, N, A), f(R, iters, N), torch.zeros(R, iters, self.n_elite, dtype=torch.int32, device=dev),
                     f(R, iters, A), f(R, iters, A))
        ops.cem_refine(embs, [s.net.head() for s in nets], self._mirrors(nets), mean0, eps, out, N, A, s1.E, s1.hidden,
                       s1.q_layers, iters, self.n_elite, self.min_std, self.max_std, self.alpha, self.discrete_gripper,
                       self.compute, trace)
        act = out[0] if unbatched else out
        if not return_trace:
            return act
        return act, dict(zip(("pop", "q", "elite", "mean", "std"), trace))
