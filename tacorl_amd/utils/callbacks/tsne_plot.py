"""The latent-plan diagnostic of PlayLMP (reference utils/callbacks/tsne_plot.py, "task_consistency"): a t-SNE map of the plans
the plan proposal samples on the validation set, coloured by the task a sequence completed.

The reference embeds with MulticoreTSNE on host cores and draws with plotly into wandb; none of the three is a dependency
here.  The embedding is tacorl_amd.evaluation.tsne.tsne_embed (exact t-SNE on the GPU; n_jobs is accepted and unused) up to
ops.TSNE_MAX_N plans and tsne_embed_neighbours (the reference library's sparse neighbour P, exact repulsion) above that; an
epoch with more than `max_points` plans is subsampled, so a whole validation set never ends the run.  The "figure" is the
data of the reference's figure: `self.last` = {"x_tsne", "labels", "shown", "kl", "step"} as host arrays, also logged as a
plain dict where the logger's experiment has `.log`."""
import logging
import math

import numpy as np
import torch

from ...lightning import CallbackBase, instantiate

log = logging.getLogger(__name__)
MAX_UNLABELLED_SHOWN = 100  # the reference's cap on "no task" points in the figure


def _gather_rows(t):
    """All ranks' rows of t (n_r, ...) in rank order, on every rank (the ranks' counts may differ)."""
    import torch.distributed as dist

    n = torch.tensor([t.shape[0]], device=t.device)
    counts = [torch.zeros_like(n) for _ in range(dist.get_world_size())]
    dist.all_gather(counts, n)
    counts = [int(c) for c in counts]
    pad = torch.zeros((max(counts),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]] = t
    parts = [torch.zeros_like(pad) for _ in counts]
    dist.all_gather(parts, pad)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0)


class TSNEPlot(CallbackBase):
    def __init__(self, perplexity, n_jobs, plot_percentage, opacity, marker_size, tasks=None, max_points=None):
        """max_points: the most plans one map embeds (None: the neighbour path's cap, ops.TSNE_NBR_MAX_N); an epoch with more
        is subsampled without replacement by self.rng."""
        self.perplexity, self.n_jobs, self.plot_percentage = perplexity, n_jobs, plot_percentage
        self.max_points = max_points
        self.opacity, self.marker_size = opacity, marker_size
        if tasks is not None and "_target_" in tasks:
            tasks = instantiate(tasks)
        get = (lambda k: tasks[k]) if isinstance(tasks, dict) else (lambda k: getattr(tasks, k))
        self.id_to_task = dict(get("id_to_task")) if tasks is not None else {}
        self.task_to_id = dict(get("task_to_id")) if tasks is not None else {}
        self.sampled_plans, self.labels = [], []
        self.last = None
        self.rng = np.random.RandomState(0)  # the figure's subsample

    # ------------------------------------------------------------------------------ collection
    def _plans(self, pl_module, outputs):
        if isinstance(outputs, dict) and "sampled_plan_pp" in outputs:
            return outputs["sampled_plan_pp"]
        if not hasattr(pl_module, "last_plan_proposal"):
            raise TypeError(f"TSNEPlot: {type(pl_module).__name__}.validation_step returns no `sampled_plan_pp` and the module "
                            "has no last_plan_proposal()")
        return pl_module.last_plan_proposal().sample()

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=0) -> None:
        plans = self._plans(pl_module, outputs)
        n = plans.shape[0]
        if isinstance(outputs, dict) and "completed_tasks" in outputs:
            # the reference's rule: sequences with more than one completed task are left out; none is label -1
            keep, labels = [], []
            for i, done in enumerate(outputs["completed_tasks"]):
                if len(done) <= 1:
                    keep.append(i)
                    labels.append(self.task_to_id[list(done)[0]] if len(done) == 1 else -1)
            plans, labels = plans[keep] if len(keep) < n else plans, torch.tensor(labels, dtype=torch.long)
        elif isinstance(batch, dict) and "task_ids" in batch:
            labels = batch["task_ids"].detach().to("cpu", torch.long).reshape(n)
        else:
            labels = torch.full((n,), -1, dtype=torch.long)
        if len(labels) > 0:
            self.sampled_plans.append(plans.detach().reshape(len(labels), -1).clone())
            self.labels.append(labels)

    # ------------------------------------------------------------------------------ the epoch's map
    def _get_tsne(self, sampled_plans):
        from ... import ops
        from ...evaluation.tsne import tsne_embed, tsne_embed_neighbours

        n = sampled_plans.reshape(-1, sampled_plans.shape[-1]).shape[0]
        embed = tsne_embed if n <= ops.TSNE_MAX_N else tsne_embed_neighbours
        return embed(sampled_plans, perplexity=self.perplexity, return_kl=True)

    def _subsample(self, plans, labels):
        """At most max_points rows of both, the kept rows in their order.  With floor(3 perplexity) > ops.TSNE_NBR_MAX_K
        (perplexity above 64) the neighbour path does not apply, so the limit is the dense path's ops.TSNE_MAX_N."""
        from ... import ops

        cap = ops.TSNE_NBR_MAX_N if self.max_points is None else min(int(self.max_points), ops.TSNE_NBR_MAX_N)
        why = "max_points"
        if ops.tsne_nbr_k(self.perplexity) > ops.TSNE_NBR_MAX_K and cap > ops.TSNE_MAX_N:
            # lists longer than the neighbour path keeps: only the dense path takes this perplexity, and it stops at its own cap
            cap, why = ops.TSNE_MAX_N, f"perplexity {self.perplexity:g} needs the dense path, which takes {ops.TSNE_MAX_N}"
        n = plans.shape[0]
        if n <= cap:
            return plans, labels
        keep = np.sort(self.rng.choice(n, size=cap, replace=False))
        log.info("TSNEPlot: %d plans this epoch, the map embeds a random %d of them (%s)", n, cap, why)
        idx = torch.from_numpy(keep)
        return plans[idx.to(plans.device)], labels[idx.to(labels.device)]

    def _shown(self, labels):
        """The rows the reference's figure shows: a plot_percentage share of each group, the unlabelled capped at 100."""
        none, task = np.where(labels == -1)[0], np.where(labels != -1)[0]
        a = self.rng.choice(none, replace=False, size=min(int(len(none) * self.plot_percentage), MAX_UNLABELLED_SHOWN))
        b = self.rng.choice(task, replace=False, size=int(len(task) * self.plot_percentage))
        return np.sort(np.concatenate([a, b]).astype(np.int64))

    def on_validation_epoch_end(self, trainer, pl_module) -> None:
        import torch.distributed as dist

        plans_l, labels_l = self.sampled_plans, self.labels
        self.sampled_plans, self.labels = [], []
        if not plans_l:
            return
        plans, labels = torch.cat(plans_l, dim=0), torch.cat(labels_l, dim=0)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            plans, labels = _gather_rows(plans), _gather_rows(labels.to(plans.device))
            if dist.get_rank() != 0:
                return
        plans, labels = self._subsample(plans, labels)
        need = math.ceil(3 * self.perplexity + 1)
        if plans.shape[0] < need:
            log.info("TSNEPlot: %d plans, perplexity %g needs at least %d: no map this epoch", plans.shape[0], self.perplexity, need)
            return
        x_tsne, kl = self._get_tsne(plans)
        labels = labels.cpu().numpy()
        step = int(getattr(pl_module, "global_step", 0))
        self.last = {"x_tsne": np.asarray(x_tsne.detach().cpu().numpy() if torch.is_tensor(x_tsne) else x_tsne),
                     "labels": labels, "shown": self._shown(labels), "kl": float(kl), "step": step}
        exp = getattr(getattr(trainer, "logger", None), "experiment", None)
        if exp is not None and hasattr(exp, "log"):
            s = self.last["shown"]
            exp.log({"task_consistency": {"x": self.last["x_tsne"][s, 0].tolist(), "y": self.last["x_tsne"][s, 1].tolist(),
                                          "label": labels[s].tolist(),
                                          "task": [self.id_to_task.get(int(i), "no task") for i in labels[s]],
                                          "opacity": self.opacity, "marker_size": self.marker_size, "kl": float(kl), "step": step}})
