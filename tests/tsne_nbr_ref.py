"""fp64 restatement of the project's neighbour-sparse t-SNE (include/tacorl_hip.h "neighbour-sparse t-SNE"; kernels:
tacorl_amd/csrc/tsne_ops.hip) and the a-priori allowances its tests hold the fp32 kernels to.  Everything the definition shares
with the dense one - normalisation, distances, the bisection, w, the update, the cost, the bounds - is tests/tsne_ref.py's.
NumPy only; every function works in the dtype of what it is given, so the same statement runs in fp32."""
import functools
import os

import numpy as np

from tests import tsne_ref as R

MAX_N, MAX_K = 131072, 192
ROW_BLOCK, MAX_SEG = 256, 32  # rows per repulsion workgroup = j per LDS tile; segments of the j range
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_nbr_clusters.npz")


# ------------------------------------------------------------------------------------------ the definition
def k_of(perplexity):
    return int(np.floor(np.float32(3) * np.float32(perplexity)))


def segment(N):
    """Segment length of the repulsion sums: the smallest multiple of 256 that cuts N into at most 32 segments."""
    return ROW_BLOCK * -(-N // (ROW_BLOCK * MAX_SEG))


def knn(xn, K):
    """(rows (N, K) int32, dists (N, K)): per row the K other rows with the smallest (d, row), ascending; d in the direct form,
    in xn's dtype.  The row itself is left out by index.  A NaN distance counts as +inf, so every list is K valid rows whatever
    the table holds (all-NaN distances: the K lowest other rows)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = R.sq_dists(xn)
    d = np.where(np.isnan(d), np.asarray(np.inf, d.dtype), d)
    N = len(d)
    others = np.arange(N - 1)[None, :] + (np.arange(N - 1)[None, :] >= np.arange(N)[:, None])  # row i: every j != i, ascending
    rows = np.take_along_axis(others, np.argsort(np.take_along_axis(d, others, 1), axis=1, kind="stable")[:, :K], 1)
    return rows.astype(np.int32), np.take_along_axis(d, rows, 1)


def list_dists(xn, rows):
    """d of every listed pair, in xn's dtype, direct form."""
    xn = np.asarray(xn)
    d = np.zeros(rows.shape, xn.dtype)
    for c in range(xn.shape[1]):
        t = xn[:, None, c] - xn[rows, c]
        d = d + t * t
    return d


def _aug(dl):
    """A list's distances as a dense-definition row: the K listed entries and, at index K, the row itself (its value is never
    used: the first neighbour's distance, so that the shifted exponent of the masked entry is 0)."""
    return np.append(dl, dl[0]), len(dl)


def row_entropy(dl, beta):
    H, p = R.row_entropy(*_aug(dl), beta)
    return H, p[:-1]


def search_beta(dl, perplexity, trace=None):
    return R.search_beta(*_aug(dl), perplexity, trace)


def conditionals(dists, perplexity):
    """(cond (N, K), betas, n_capped) of the listed distances."""
    res = [search_beta(dl, perplexity) for dl in dists]
    betas = np.array([r[0] for r in res], dtype=dists.dtype)
    return cond_rows(dists, betas), betas, sum(r[1] for r in res)


def cond_rows(dists, betas):
    return np.stack([row_entropy(dl, b)[1] for dl, b in zip(dists, betas)])


def scatter(rows, cond):
    """Dense (N, N) conditionals and their pattern (for the small tables of the tests)."""
    N = len(rows)
    C, M = np.zeros((N, N), cond.dtype), np.zeros((N, N), bool)
    i = np.arange(N)[:, None]
    C[i, rows], M[i, rows] = cond, True
    return C, M


def csr(rows, cond):
    """(row_ptr, col, val): row i holds every j with j in N(i) or i in N(j), ascending; val = (a + b) / (2 N), one addition and
    one division in cond's dtype."""
    N, dt = len(rows), cond.dtype.type
    C, M = scatter(rows, cond)
    P = (C + C.T) / (dt(2) * dt(N))
    pat = M | M.T
    row_ptr = np.concatenate([[0], np.cumsum(pat.sum(1))]).astype(np.int32)
    ri, ci = np.nonzero(pat)  # row-major: ascending columns inside a row
    return row_ptr, ci.astype(np.int32), P[ri, ci]


def dense(row_ptr, col, val, dtype=None):
    """The CSR as a dense (N, N) matrix: with it forces, step, kl and run are tests/tsne_ref.py's (its repulsion and Z run over
    all pairs whatever P holds, its cost over the entries P > 0)."""
    N = len(row_ptr) - 1
    P = np.zeros((N, N), dtype or val.dtype)
    P[np.repeat(np.arange(N), np.diff(row_ptr)), col[:row_ptr[N]]] = val[:row_ptr[N]]
    return P


def affinities(X, perplexity, dtype=np.float64):
    """(row_ptr, col, val, rows, dists, cond, betas, n_capped) from the raw table."""
    xn = R.normalise(X, dtype)
    rows, dists = knn(xn, k_of(perplexity))
    cond, betas, capped = conditionals(dists, perplexity)
    return (*csr(rows, cond), rows, dists, cond, betas, capped)


def forces_rows(row_ptr, col, val, Y, rows):
    """fp64 (attr, rep, Z_i, sum|attr terms|, sum|rep terms|, sum|Z terms|, entries) of the given rows only."""
    Y = np.asarray(Y, np.float64)
    out = [[] for _ in range(7)]
    for i in rows:
        diff = Y[i] - Y
        w = 1 / (1 + (diff * diff).sum(1))
        w[i] = 0
        tr = (w * w)[:, None] * diff
        e = slice(row_ptr[i], row_ptr[i + 1])
        ta = (val[e].astype(np.float64) * w[col[e]])[:, None] * diff[col[e]]
        for o, v in zip(out, (ta.sum(0), tr.sum(0), w.sum(), np.abs(ta).sum(0), np.abs(tr).sum(0), w.sum(), e.stop - e.start)):
            o.append(v)
    return [np.array(o) for o in out]


def _wave_rows_csr(row_ptr, T):
    """Row sums of the per-entry terms T in the definition's order: lane l adds the row's entries l, l + 64, ... in order, then
    the xor butterfly 32 .. 1."""
    N, dt = len(row_ptr) - 1, T.dtype
    M = -(-int(np.diff(row_ptr).max()) // 64)
    pad = np.zeros((N, M * 64), dt)
    lens = np.diff(row_ptr)
    pad[np.repeat(np.arange(N), lens), np.arange(row_ptr[N]) - np.repeat(row_ptr[:-1], lens)] = T[:row_ptr[N]]
    acc = np.zeros((N, 64), dt)
    for k in range(M):
        acc = acc + pad[:, 64 * k:64 * k + 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def _segment_rows(T):
    """Row sums of T (N, N) in the repulsion's order: inside a segment ascending j from 0, then the segments ascending from 0."""
    N, L = T.shape[0], segment(T.shape[0])
    acc = np.zeros(N, T.dtype)
    for j0 in range(0, N, L):
        s = np.zeros(N, T.dtype)
        for j in range(j0, min(j0 + L, N)):
            s = s + T[:, j]
        acc = acc + s
    return acc


def step_in_kernel_order(row_ptr, col, val, Y, u, gains, ex, mom, lr):
    """One iteration with every sum in the order the definition states, in Y's dtype."""
    dt, N = Y.dtype.type, len(Y)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    w = dt(1) / (dt(1) + (dx * dx + dy * dy))
    np.fill_diagonal(w, 0)
    w2 = w * w
    ri = np.repeat(np.arange(N), np.diff(row_ptr))
    ci = col[:row_ptr[N]]
    pw = val[:row_ptr[N]].astype(Y.dtype) * w[ri, ci]
    attr = np.stack([_wave_rows_csr(row_ptr, pw * dx[ri, ci]), _wave_rows_csr(row_ptr, pw * dy[ri, ci])], 1)
    rep = np.stack([_segment_rows(w2 * dx), _segment_rows(w2 * dy)], 1)
    Z = R._tree_1024(_segment_rows(w))
    g = dt(4) * (dt(ex) * attr - rep / Z)
    gains = np.maximum(np.where((g > 0) != (u > 0), gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    u = dt(mom) * u - dt(lr) * (gains * g)
    Y = Y + u
    mean = np.array([R._tree_1024(Y[:, 0]), R._tree_1024(Y[:, 1])], Y.dtype) / dt(N)
    return Y - mean, u, gains


# ------------------------------------------------------------------------------------------ allowances
# The bisection, e_s, S and the division are the dense row's over K + 1 "columns" (the list and the row itself), so the dense
# allowances apply to a list as they stand: a wave adds at most ceil(K / 64) <= wave_depth(K + 1) - 6 terms per lane.
def entropy_allowance(dl, beta, D):
    return R.entropy_allowance(*_aug(dl), beta, D)


def cond_allowance(dl, beta, D):
    return R.cond_allowance(*_aug(dl), beta, D)[:-1]


def val_allowance(rows, dists, betas, D):
    """Per stored entry of P, in CSR order: the two conditional allowances (zero where the half is absent: an absent half is an
    exact 0), plus the addition and the division - tsne_ref.p_allowance on the pattern."""
    N = len(rows)
    ca = np.stack([cond_allowance(dl, b, D) for dl, b in zip(dists, betas)])
    A, M = scatter(rows, ca)
    C, _ = scatter(rows, cond_rows(dists, betas))
    allow = (A + A.T + 2 * R.U * (C + C.T)) / (2 * N) + R.TINY
    return allow[M | M.T]


# ------------------------------------------------------------------------------------------ data
def ties_table(N, D, seed):
    """Groups of four identical rows (a ragged last group): every row has duplicates at d = 0, ties at every list position."""
    rs = np.random.RandomState(seed)
    return np.repeat(rs.uniform(-1, 1, (-(-N // 4), D)).astype(np.float32), 4, axis=0)[:N].copy()


def hub_table(N=300, D=32, seed=5):
    """One centre point (row 0) and N - 1 points on a wide shell around it, far from each other: the centre is in every list."""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((N, D))
    X = v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.01 * rs.standard_normal((N, 1)))
    X[0] = 0
    return X.astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden():
    G = np.load(GOLDEN)
    out = {k: G[k] for k in G.files}
    for v in out.values():
        v.setflags(write=False)
    return out
