"""What the device-noise tests share: the fp32 error bound of a normal draw against the fp64 restatement
(tacorl_amd.noise.philox_restatement), planted defects that the bound must tell from rounding, the standardised moment
statistics, and a small carver of test segment tables.  NumPy only.

The bound.  The kernel computes z = r * c with r = sqrtf(-2 logf(u1)) and (s, c) = sincospif(2 u2); u1, 2 u2 and the factor 2
are exact.  With relative errors d_log, d_sqrt, d_sc of the three functions and d_mul <= 2^-24 of the final product,

    z = z_exact * sqrt(1 + d_log) * (1 + d_sqrt) * (1 + d_sc) * (1 + d_mul)
      ~ z_exact * (1 + d_log / 2 + d_sqrt + d_sc + d_mul)

so |z - z_exact| <= (E_LOG / 2 + E_SQRT + E_SINCOS + 1 / 2) * 2^-23 * |z_exact| with the E_* in units of 2^-23.  The E_* are the
maxima that tools/noise_math_probe.hip measured on the device over the kernel's WHOLE domain (every 24-bit u1 and u2; recorded
in profiles/device_noise.md) - no copy of the HIP math accuracy table ships with the toolchain -, rounded up.  The bound doubles
the propagated sum and has the form K * 2^-23 * max(|z|, 1).
"""
import numpy as np

from tacorl_amd import noise as N

E_LOG, E_SQRT, E_SINCOS = 1.35, 0.5, 0.73  # units of 2^-23 (relative); measured 1.3459, 0.5000, 0.7268
K_SUM = E_LOG / 2 + E_SQRT + E_SINCOS + 0.5
K = 2.0 * K_SUM


def normal_bound(z64):
    return K * 2.0 ** -23 * np.maximum(np.abs(z64), 1.0)


# ------------------------------------------------------------------------------------------------ planted defects
def _box_muller(a, b, bits=24, swap=False):
    sh = np.uint32(32 - bits)
    u1 = ((a >> sh).astype(np.float64) + 1.0) * 2.0 ** -bits
    th = 2.0 * np.pi * (b >> sh).astype(np.float64) * 2.0 ** -bits
    r = np.sqrt(-2.0 * np.log(u1))
    return (r * np.sin(th), r * np.cos(th)) if swap else (r * np.cos(th), r * np.sin(th))


def defective_normals(words, defect):
    """fp64 normals from (..., 4) words with one defect planted: 'swap' (sin and cos exchanged), 'bits23' (23-bit uniforms),
    'pairs02' (word pairs (0,2), (1,3) instead of (0,1), (2,3)); None: the restatement itself."""
    w = np.asarray(words, dtype=np.uint32)
    pairs = ((0, 2), (1, 3)) if defect == "pairs02" else ((0, 1), (2, 3))
    out = np.empty(w.shape, dtype=np.float64)
    for i, (pa, pb) in enumerate(pairs):
        out[..., 2 * i], out[..., 2 * i + 1] = _box_muller(w[..., pa], w[..., pb], 23 if defect == "bits23" else 24,
                                                             defect == "swap")
    return out


# ------------------------------------------------------------------------------------------------ moments
def normal_stats(x):
    """Standardised mean, variance and fourth moment of n supposed N(0, 1) draws (each ~ N(0, 1) under the hypothesis)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    return {"mean": x.mean() * np.sqrt(n), "var": ((x * x).mean() - 1.0) / np.sqrt(2.0 / n),
            "m4": ((x ** 4).mean() - 3.0) / np.sqrt(96.0 / n)}


def uniform_stats(u):
    u = np.asarray(u, dtype=np.float64).ravel()
    n = u.size
    return {"mean": (u.mean() - 0.5) / np.sqrt(1.0 / (12.0 * n)),
            "var": (((u - 0.5) ** 2).mean() - 1.0 / 12.0) / np.sqrt(1.0 / (180.0 * n))}


def corr_stat(x, y):
    """Standardised correlation of two supposed independent N(0, 1) arrays (the product has mean 0 and variance 1)."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    return (x * y).mean() * np.sqrt(x.size)


# ------------------------------------------------------------------------------------------------ test tables
def al4(x):
    return (x + 3) // 4 * 4


def carve(specs, pad=4):
    """specs: (kind, draw_id, B_local, inner, n_outer, outer_major[, keep_p]) -> (SegmentTable, n_f32, n_u8): buffers carved
    like the engine's (every buffer starts on a multiple of 4 elements; `pad` more untouched elements behind each)."""
    segs, off = [], {False: 0, True: 0}
    for sp in specs:
        kind, did, B, inner, n_outer, om = sp[:6]
        u8 = kind == "keep"
        s = N.Segment(off[u8], kind, did, B, inner, n_outer, om, keep_p=sp[6] if u8 else 0.0)
        segs.append(s)
        off[u8] = al4(off[u8] + s.numel) + pad
    return N.SegmentTable(segs, max(off[False], 4), off[True]), max(off[False], 4), off[True]


def expected(seg, seed, step, sample0):
    return N.philox_restatement(seed, step, seg.draw_id, seg.kind, seg.B_local, seg.inner, seg.n_outer, sample0, seg.outer_major,
                                seg.keep_p)
