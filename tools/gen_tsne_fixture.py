"""Generate tests/golden/tsne_clusters.npz from the fp64 restatement of the project's exact t-SNE (tests/tsne_ref.py):

    python tools/gen_tsne_fixture.py

  X, labels         the clustered table (6 clusters x 40 points, 16 dimensions, perplexity 30)
  inits (8, N, 2)   eight initialisations 1e-4 N(0, 1)
  kl0, kl (8)       fp64 cost at inits[k] and after the 1000 iterations from it;  acc (8): 5-NN label accuracy of each result
  mid_<N>           for every N of the GPU force cases (tsne_ref.case_table(N, 16, seed N)): the state (Y, u, gains) in front of
                    iteration 300 of the fp64 run from a seeded init, rounded to fp32 - exaggeration off, momentum 0.8, spread gains
No reference program takes part: the definition is this project's own."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_ref as R  # noqa: E402

PERPLEXITY = 30.0
FORCE_N = (16, 63, 64, 65, 255, 257, 1000)


def main():
    X, labels = R.clusters()
    P, betas, capped, d = R.affinities(X, PERPLEXITY)
    assert capped == 0
    rs = np.random.RandomState(1)
    inits = 1e-4 * rs.standard_normal((8, len(X), 2))
    kl0, klf, acc = [], [], []
    for k in range(8):
        Y = R.run(P, inits[k])
        kl0.append(R.kl(P, inits[k])), klf.append(R.kl(P, Y)), acc.append(R.knn_accuracy(Y, labels))
        print(f"init {k}: KL {kl0[-1]:.4f} -> {klf[-1]:.4f}, 5-NN accuracy {acc[-1]:.3f}", flush=True)
    out = dict(X=X, labels=labels, perplexity=np.array(PERPLEXITY), inits=inits, kl0=np.array(kl0), kl=np.array(klf),
               acc=np.array(acc))
    for N in FORCE_N:
        t0 = time.time()
        Pn = R.affinities(R.case_table(N, 16, N), R.perplexity_for(N))[0]
        Y0 = 1e-4 * np.random.RandomState(N).standard_normal((N, 2))
        _, kept = R.run(Pn, Y0, n_iter=301, keep=(300,))
        out[f"mid_{N}"] = np.stack(kept[300]).astype(np.float32)
        g = kept[300][2]
        print(f"N = {N}: gains {g.min():.3g} .. {g.max():.3g}, |Y| max {np.abs(kept[300][0]).max():.3g}, {time.time() - t0:.1f} s",
              flush=True)
    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
