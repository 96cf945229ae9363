"""Generate tests/golden/tsne_nbr_clusters.npz from the fp64 restatement of the project's neighbour-sparse t-SNE
(tests/tsne_nbr_ref.py):

    python tools/gen_tsne_nbr_golden.py

  kl0, kl (8)       fp64 cost of THIS definition at tsne_clusters.npz's inits[k] and after the 1000 iterations from it, on that
                    fixture's table at its perplexity (X, labels, inits are read from there, not copied);  acc (8): 5-NN label
                    accuracy of each result
  mid_<N>           for the N of the GPU force cases that tsne_clusters.npz has no state for (tsne_ref.case_table(N, 16, seed N)
                    at tsne_ref.perplexity_for(N)): the state (Y, u, gains) in front of iteration 300 of the fp64 run from a
                    seeded init, rounded to fp32
No reference program takes part: the definition is this project's own."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tsne_nbr_ref as NR  # noqa: E402
from tests import tsne_ref as R  # noqa: E402

FORCE_N = (121, 256)


def main():
    G = R.golden()
    a = NR.affinities(G["X"], float(G["perplexity"]))
    assert a[-1] == 0
    P = NR.dense(*a[:3])
    kl0, klf, acc = [], [], []
    for k, Y0 in enumerate(G["inits"]):
        Y = R.run(P, Y0)
        kl0.append(R.kl(P, Y0)), klf.append(R.kl(P, Y)), acc.append(R.knn_accuracy(Y, G["labels"]))
        print(f"init {k}: KL {kl0[-1]:.4f} -> {klf[-1]:.4f}, 5-NN accuracy {acc[-1]:.3f}", flush=True)
    out = dict(perplexity=np.array(float(G["perplexity"])), kl0=np.array(kl0), kl=np.array(klf), acc=np.array(acc))
    for N in FORCE_N:
        t0 = time.time()
        Pn = NR.dense(*NR.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[:3])
        Y0 = 1e-4 * np.random.RandomState(N).standard_normal((N, 2))
        _, kept = R.run(Pn, Y0, n_iter=301, keep=(300,))
        out[f"mid_{N}"] = np.stack(kept[300]).astype(np.float32)
        g = kept[300][2]
        print(f"N = {N}: gains {g.min():.3g} .. {g.max():.3g}, |Y| max {np.abs(kept[300][0]).max():.3g}, {time.time() - t0:.1f} s",
              flush=True)
    np.savez_compressed(NR.GOLDEN, **out)
    print("wrote", NR.GOLDEN, os.path.getsize(NR.GOLDEN) / 1e3, "kB")


if __name__ == "__main__":
    main()
