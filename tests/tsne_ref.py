"""fp64 restatement of the project's exact t-SNE (include/tacorl_hip.h "exact t-SNE"; kernels: tacorl_amd/csrc/tsne_ops.hip) and
the a-priori error allowances its tests hold the fp32 kernels to.  NumPy only; every function takes a dtype so that the same
statement can be run in fp32 (the deviation the short-trajectory tests scale their tolerance from).

u = 2^-24 is the fp32 unit roundoff throughout."""
import functools
import os

import numpy as np

U = 2.0 ** -24
TOL_H = 1e-5
MAX_STEPS = 200
TINY = 2.0 ** -126
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_clusters.npz")


# ------------------------------------------------------------------------------------------ the definition
def normalise(X, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    xc = X - X.sum(axis=0, dtype=dtype) / dtype(len(X))
    m = np.abs(xc).max()
    if m == 0:
        raise ValueError("t-SNE of an all-equal table")
    return xc / m


def sq_dists(xn):
    """Direct form, sequentially over the columns, in xn's dtype."""
    xn = np.asarray(xn)
    d = np.zeros((len(xn), len(xn)), dtype=xn.dtype)
    for c in range(xn.shape[1]):
        t = xn[:, None, c] - xn[None, :, c]
        d = d + t * t
    return d


def row_entropy(drow, i, beta):
    """(H, p): entropy and conditional row of row i at beta, shifted by the row's smallest off-diagonal distance."""
    dt = drow.dtype.type
    mask = np.ones(len(drow), bool)
    mask[i] = False
    t = drow - drow[mask].min()
    e = np.where(mask, np.exp(-(dt(beta) * t)), dt(0))
    S = e.sum(dtype=dt)
    H = np.log(S) + dt(beta) * (e * t).sum(dtype=dt) / S
    return H, e / S


def search_beta(drow, i, perplexity, trace=None):
    """The bisection of the definition.  Returns (beta, capped)."""
    dt = drow.dtype.type
    target = np.log(dt(perplexity))
    beta, lo, hi = dt(1), None, None
    for step in range(MAX_STEPS):
        if trace is not None:
            trace.append(beta)
        H, _ = row_entropy(drow, i, beta)
        diff = H - target
        if abs(diff) < TOL_H:
            return beta, False
        if step == MAX_STEPS - 1:
            return beta, True
        if diff > 0:
            lo = beta
            beta = (beta + hi) / dt(2) if hi is not None else min(beta * dt(2), dt(1e30))
        else:
            hi = beta
            beta = (beta + lo) / dt(2) if lo is not None else beta / dt(2)
    raise AssertionError


def cond_rows(d, betas):
    return np.stack([row_entropy(d[i], i, betas[i])[1] for i in range(len(d))])


def symmetrise(cond):
    return (cond + cond.T) / cond.dtype.type(2 * len(cond))


def affinities(X, perplexity, dtype=np.float64):
    """(P, beta, n_capped, d) from the raw table."""
    d = sq_dists(normalise(X, dtype))
    res = [search_beta(d[i], i, perplexity) for i in range(len(d))]
    betas = np.array([r[0] for r in res], dtype=dtype)
    return symmetrise(cond_rows(d, betas)), betas, sum(r[1] for r in res), d


def forces(P, Y):
    """attr (N, 2), rep (N, 2), Zi (N) and the per-row sums of |term| of each (the Higham bound's right-hand side)."""
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1 / (1 + (diff * diff).sum(-1, dtype=Y.dtype))
    np.fill_diagonal(w, 0)
    ta, tr = (P * w)[:, :, None] * diff, (w * w)[:, :, None] * diff
    return (ta.sum(1, dtype=Y.dtype), tr.sum(1, dtype=Y.dtype), w.sum(1, dtype=Y.dtype),
            np.abs(ta).sum(1), np.abs(tr).sum(1), np.abs(w).sum(1))


def step(P, Y, u, gains, ex, mom, lr):
    """One iteration; returns new (Y, u, gains)."""
    dt = Y.dtype.type
    attr, rep, zi = forces(P, Y)[:3]
    g = dt(4) * (dt(ex) * attr - rep / zi.sum(dtype=Y.dtype))
    gains = np.maximum(np.where((g > 0) != (u > 0), gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    u = dt(mom) * u - dt(lr) * (gains * g)
    Y = Y + u
    return Y - Y.sum(0, dtype=Y.dtype) / dt(len(Y)), u, gains


def _wave_rows(T):
    """Row sums of T (N, N) in the order the definition gives a row's wave: lane l adds j = 4 l + 256 k + {0, 1, 2, 3} in order
    (absent and diagonal entries are zero terms here, skipped there: the same value), then the xor butterfly 32 .. 1."""
    N, dt = len(T), T.dtype
    K = -(-N // 256)
    pad = np.zeros((N, K * 256), dt)
    pad[:, :N] = T
    pad = pad.reshape(N, K, 64, 4)
    acc = np.zeros((N, 64), dt)
    for k in range(K):
        for m in range(4):
            acc = acc + pad[:, k, :, m]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def _tree_1024(v):
    """The one-workgroup sum of the definition: thread t of 1024 adds v[t], v[t + 1024], ... in order, then strides 512 .. 1."""
    dt = v.dtype
    M = -(-len(v) // 1024)
    pad = np.zeros(M * 1024, dt)
    pad[:len(v)] = v
    s = np.zeros(1024, dt)
    for r in pad.reshape(M, 1024):
        s = s + r
    h = 512
    while h:
        s = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def step_in_kernel_order(P, Y, u, gains, ex, mom, lr):
    """`step` with every sum taken in the order include/tacorl_hip.h states for it, in Y's dtype: run in fp32 this is the
    definition as an fp32 machine evaluates it (the deviation the short-trajectory tests scale their tolerance from)."""
    dt = Y.dtype.type
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    w = dt(1) / (dt(1) + (dx * dx + dy * dy))
    np.fill_diagonal(w, 0)
    pw, w2 = P * w, w * w
    attr = np.stack([_wave_rows(pw * dx), _wave_rows(pw * dy)], 1)
    rep = np.stack([_wave_rows(w2 * dx), _wave_rows(w2 * dy)], 1)
    Z = _tree_1024(_wave_rows(w))
    g = dt(4) * (dt(ex) * attr - rep / Z)
    gains = np.maximum(np.where((g > 0) != (u > 0), gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    u = dt(mom) * u - dt(lr) * (gains * g)
    Y = Y + u
    mean = np.array([_tree_1024(Y[:, 0]), _tree_1024(Y[:, 1])], Y.dtype) / dt(len(Y))
    return Y - mean, u, gains


def schedule(it,early_exaggeration=12.0, n_iter_early_exag=250):
    return (early_exaggeration, 0.5) if it < n_iter_early_exag else (1.0, 0.8)


def run(P, Y0, n_iter=1000, lr=200.0, keep=()):
    """The whole optimisation from Y0; `keep`: iterations whose state (Y, u, gains) BEFORE the iteration is returned too."""
    Y, u, gains = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    kept = {}
    for it in range(n_iter):
        if it in keep:
            kept[it] = (Y.copy(), u.copy(), gains.copy())
        ex, mom = schedule(it)
        Y, u, gains = step(P, Y, u, gains, ex, mom, lr)
    return (Y, kept) if keep else Y


def kl(P, Y):
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1 / (1 + (diff * diff).sum(-1))
    np.fill_diagonal(w, 0)
    pos = P > 0
    return float((P[pos] * np.log(P[pos] / (w[pos] / w.sum()))).sum())


def knn_accuracy(Y, labels, k=5):
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nb = labels[np.argsort(d, axis=1, kind="stable")[:, :k]]
    votes = np.stack([(nb == c).sum(1) for c in range(int(labels.max()) + 1)], 1)
    return float((votes.argmax(1) == labels).mean())


# ------------------------------------------------------------------------------------------ allowances
def sum_bound(n, abs_terms):
    """Higham, Accuracy and Stability, eq. 3.5 (as mlp_ref.lin_bound), with 8 added to the count for the roundings inside a term: any order of n fp32 additions of terms that
    carry a few roundings each - |fl(sum) - sum| <= (n + 8) u sum|term|."""
    return (n + 8) * U * abs_terms


def wave_depth(N):
    """Additions on the longest path of a row sum of the affinity kernel: ceil(N / 64) per lane, then 6 butterfly steps."""
    return -(-N // 64) + 6


def normalise_allowance(X):
    """|xn_fp32 - xn_fp64| per element.  The column sum (any order) is within (N + 8) u sum|x|, so the mean within that / N + u |mean|;
    the subtraction, the maximum (a selection) and the division add one rounding each on values <= 1 after the division; the
    error of M itself (the error of one centred element) is relative to M and scales every element by (1 + that)."""
    X = np.asarray(X, np.float64)
    xc = X - X.mean(0)
    M = np.abs(xc).max()
    dmean = sum_bound(len(X), np.abs(X).sum(0)) / len(X) + U * np.abs(X.mean(0))
    dxc = dmean[None, :] + U * np.abs(xc)          # one centred element
    return dxc / M + (dxc.max() / M + 2 * U) * np.abs(xc) / M + U


def _row_terms(drow, i, beta, D):
    """fp64 quantities of row i at beta that the allowances are made of.  delta_j bounds the relative error of the kernel's
    e_j: the distance (D + 3 roundings of a direct-form sum of D non-negative terms, so (D + 3) u d_ij absolute, which the
    exponent scales by beta - the error of the row minimum itself is common to all j and cancels in p), the subtraction of the
    minimum and the product with beta (one rounding each on the exponent x_j: 2 u x_j) and expf (2 u)."""
    mask = np.ones(len(drow), bool)
    mask[i] = False
    dmin = drow[mask].min()
    x = beta * (drow - dmin)
    e = np.where(mask, np.exp(-x), 0.0)
    S = e.sum()
    p = e / S
    m = (p * x).sum()
    delta = U * ((D + 3) * beta * drow + 2 * x + 2)
    return x, p, m, np.log(S) + m, delta


def entropy_allowance(drow, i, beta, D):
    """|H_kernel(beta) - H_fp64(beta)| + the search tolerance, for a row whose search converged.
    H = log S + m, m = sum p_j x_j.  A relative error delta_j on e_j moves H by sum p_j delta_j (1 + |x_j - m|) at first
    order (d log S = sum p_j delta_j; dm = sum p_j delta_j (x_j - m)); the error of t_j inside the weighted sum moves m by
    sum p_j (D + 4) u beta d_ij; the two sums (depth wave_depth(N), products e_j t_j rounded once) move log S and m by
    (depth + 8) u (1 + 2 m); logf, the product with beta, the division and the final addition: 4 u (1 + H)."""
    N = len(drow)
    x, p, m, H, delta = _row_terms(drow, i, beta, D)
    first = (p * delta * (1 + np.abs(x - m))).sum() + (p * (D + 4) * U * beta * drow).sum()
    return TOL_H + first + sum_bound(wave_depth(N), 1 + 2 * m) + 4 * U * (1 + H)


def cond_allowance(drow, i, beta, D):
    """Per element of the conditional row: p_j (delta_j + relative error of S + one division), and the fp32 underflow
    threshold (an e_j or a quotient below 2^-126 may be flushed to zero)."""
    N = len(drow)
    x, p, m, H, delta = _row_terms(drow, i, beta, D)
    dS = (p * delta).sum() + sum_bound(wave_depth(N), 1.0)
    return p * (delta + dS + U) + TINY


def p_allowance(d, betas, D):
    """Per element of P = (c + c^T) / 2N: the two conditional allowances, plus the addition and the division."""
    N = len(d)
    ca = np.stack([cond_allowance(d[i], i, betas[i], D) for i in range(N)])
    c = cond_rows(d, betas)
    return (ca + ca.T + 2 * U * (c + c.T)) / (2 * N) + TINY


# ------------------------------------------------------------------------------------------ data
def clusters(seed=0, n_clusters=6, per=40, dim=16, noise=0.15):
    """The fixture's table: tanh of cluster centres U(-0.8, 0.8) + N(0, noise) pre-images (latent plans are tanh outputs)."""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-0.8, 0.8, (n_clusters, dim))
    labels = np.repeat(np.arange(n_clusters), per)
    X = np.tanh(centres[labels] + noise * rs.standard_normal((len(labels), dim))).astype(np.float32)
    return X, labels


def case_table(N, D, seed, duplicates=False):
    """Test tables of the GPU cases: four loose clusters, so that rows have neighbours at several scales."""
    rs = np.random.RandomState(seed)
    X = (rs.uniform(-1, 1, (4, D))[rs.randint(0, 4, N)] + 0.3 * rs.standard_normal((N, D))).astype(np.float32)
    if duplicates:
        X[1], X[N - 1], X[N // 2] = X[0], X[2], X[2]  # a pair and a triple of identical rows
    return X


def perplexity_for(N):
    return 5.0 if N < 100 else 40.0


@functools.lru_cache(maxsize=None)
def golden():
    G = np.load(GOLDEN)
    out = {k: G[k] for k in G.files}
    for v in out.values():
        v.setflags(write=False)
    return out
