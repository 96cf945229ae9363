"""Exact t-SNE of latent plans on the GPU (the embedding behind the reference's TSNEPlot callback, which calls
MulticoreTSNE(n_jobs=8) on host cores: utils/callbacks/tsne_plot.py:100-104).  Definition: include/tacorl_hip.h "exact t-SNE";
it is this project's own (exact, dense P, van der Maaten's optimiser constants) and not bit-comparable with that Barnes-Hut
library.  All arithmetic is tsne_ops.hip's; this file allocates once and issues the launches."""
import torch

from .. import _lib as L
from .. import ops


def tsne_embed(plans, perplexity=40.0, n_iter=1000, lr=200.0, early_exaggeration=12.0, n_iter_early_exag=250, init=None,
               generator=None, return_kl=False):
    """plans: (N, A) or (..., A) fp32 device tensor -> (N, 2) fp32 on the same device (and the final KL as a float with
    return_kl).  init: (N, 2) start, else 1e-4 N(0, 1) from `generator` (a device generator) or torch's default one.
    Nothing is read back inside the loop: the status word (and the KL) cross to the host after it.
    ValueError for an all-equal table; TacorlHipError where N, A or the perplexity is outside the kernel's range."""
    if not (torch.is_tensor(plans) and plans.is_cuda):
        raise L.TacorlHipError("tsne_embed: the plans must be a device tensor (there is no host path)")
    X = plans.detach().reshape(-1, plans.shape[-1]).to(torch.float32).contiguous()
    N, D = X.shape
    dev = X.device
    if not ops.tsne_supported(N, D) or not (perplexity >= 1.0 and 3.0 * perplexity <= N - 1):
        raise L.TacorlHipError(f"tsne_embed: N = {N} (4..{ops.TSNE_MAX_N}), A = {D} (1..{ops.TSNE_MAX_D}), perplexity = "
                               f"{perplexity} (1 <= perplexity, 3 * perplexity <= N - 1) not supported")
    if init is not None:
        Y = init.detach().to(device=dev, dtype=torch.float32).reshape(N, 2).clone()
    else:
        Y = torch.randn(N, 2, device=dev, generator=generator).mul_(1e-4)
    u, gains = torch.zeros(N, 2, device=dev), torch.ones(N, 2, device=dev)
    P, _, status, ws = ops.tsne_affinities(X, perplexity)
    for it in range(int(n_iter)):
        early = it < n_iter_early_exag
        ops.tsne_step(P, Y, u, gains, early_exaggeration if early else 1.0, 0.5 if early else 0.8, lr, ws)
    kl = ops.tsne_kl(P, Y, ws) if return_kl else None
    capped, degenerate = status.tolist()
    if degenerate:
        raise ValueError("tsne_embed: every row of the table is the same point")
    if capped:
        raise L.TacorlHipError(f"tsne_embed: the perplexity search of {capped} row(s) ended at its step cap "
                               "(more identical rows than the perplexity admits?)")
    return (Y, float(kl.item())) if return_kl else Y


def tsne_embed_neighbours(plans, perplexity=40.0, n_iter=1000, lr=200.0, early_exaggeration=12.0, n_iter_early_exag=250, init=None,
                          generator=None, return_kl=False):
    """tsne_embed by the neighbour-sparse definition (include/tacorl_hip.h "neighbour-sparse t-SNE": the reference library's
    P over the floor(3 perplexity) nearest neighbours as CSR, exact repulsion, nothing of size N x N) - for tables above the
    dense path's ops.TSNE_MAX_N rows, up to ops.TSNE_NBR_MAX_N.  Arguments, returns and errors are tsne_embed's; nothing is
    read back inside the loop."""
    if not (torch.is_tensor(plans) and plans.is_cuda):
        raise L.TacorlHipError("tsne_embed_neighbours: the plans must be a device tensor (there is no host path)")
    X = plans.detach().reshape(-1, plans.shape[-1]).to(torch.float32).contiguous()
    N, D = X.shape
    dev = X.device
    K = ops.tsne_nbr_k(perplexity) if perplexity >= 1.0 else 0
    if not ops.tsne_nbr_supported(N, D, K):
        raise L.TacorlHipError(f"tsne_embed_neighbours: N = {N} (4..{ops.TSNE_NBR_MAX_N}), A = {D} (1..{ops.TSNE_MAX_D}), "
                               f"perplexity = {perplexity} (1 <= perplexity, floor(3 * perplexity) <= min(N - 1, "
                               f"{ops.TSNE_NBR_MAX_K})) not supported")
    if init is not None:
        Y = init.detach().to(device=dev, dtype=torch.float32).reshape(N, 2).clone()
    else:
        Y = torch.randn(N, 2, device=dev, generator=generator).mul_(1e-4)
    u, gains = torch.zeros(N, 2, device=dev), torch.ones(N, 2, device=dev)
    a = ops.tsne_nbr_affinities(X, perplexity)
    csr, ws = (a["row_ptr"], a["col"], a["val"]), a["ws"]
    for it in range(int(n_iter)):
        early = it < n_iter_early_exag
        ops.tsne_nbr_step(*csr, Y, u, gains, early_exaggeration if early else 1.0, 0.5 if early else 0.8, lr, ws)
    kl = ops.tsne_nbr_kl(*csr, Y, ws) if return_kl else None
    capped, degenerate = a["status"].tolist()
    if degenerate:
        raise ValueError("tsne_embed_neighbours: every row of the table is the same point")
    if capped:
        raise L.TacorlHipError(f"tsne_embed_neighbours: the perplexity search of {capped} row(s) ended at its step cap "
                               "(more identical rows than the perplexity admits?)")
    return (Y, float(kl.item())) if return_kl else Y
