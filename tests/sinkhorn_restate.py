"""numpy restatement of the Sinkhorn / inverted-softmax potentials (kiez_amd.hubness_reduction.Sinkhorn, InvertedSoftmax;
kz_softmin_rows), float64 throughout.  D is the [n_s, n_t] matrix of the distances the search returns; eps > 0 the temperature.

    softmin_eps(x) = m - eps log sum exp(-(x - m) / eps),   m = min x
    Sinkhorn from f = 0, L times:   g_j = softmin_eps over i of (D_ij - f_i) + eps log(n_s / n_t)      (column step)
                                    f_i = softmin_eps over j of (D_ij - g_j)                            (row step)
    inverted softmax:               g_j = softmin_eps over i of D_ij,  f = 0
    w_ij = (D_ij - f_i) - g_j

A NaN entry counts as +inf; a set without an entry below +inf gives +inf, one with a -inf gives -inf."""
import numpy as np


def softmin(x, eps, axis=-1):
    """The min-shifted soft-min along `axis`."""
    x = np.where(np.isnan(x), np.inf, np.asarray(x, dtype=np.float64))
    m = x.min(axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.exp(-((x - m) / eps)).sum(axis=axis, keepdims=True)   # (inf - inf = NaN where m is infinite: replaced below)
        out = m - eps * np.log(s)
    return np.where(np.isinf(m), m, out).squeeze(axis)


def sinkhorn_potentials(D, eps, L):
    """(f [n_s], g [n_t]) after L iterations."""
    n_s, n_t = D.shape
    f = np.zeros(n_s)
    g = np.zeros(n_t)
    for _ in range(L):
        g = softmin(D - f[:, None], eps, axis=0) + eps * np.log(n_s / n_t)
        f = softmin(D - g[None, :], eps, axis=1)
    return f, g


def inverted_softmax_potential(D, eps):
    """g [n_t]: one column step from f = 0, without the constant."""
    return softmin(D, eps, axis=0)


def w(D, f, g):
    return (D - f[:, None]) - g[None, :]


def bracket(want, eps):
    """What one soft-min may differ by: 1e-12 (|want| + eps).  A different summation order costs a relative ~log2(n) 2^-53 on the sum,
    an absolute eps 2e-15 on the result, plus one rounding of m."""
    return 1e-12 * (np.abs(want) + eps)


def alignment_case(n_s, n_t, noise, d=16, seed=0):
    """The generator of the fit tests: noisy copies of a random subset of unit target rows.  -> source, target, gold."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n_t, d))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    perm = rng.permutation(n_t)[:n_s]
    s = t[perm] + noise * rng.standard_normal((n_s, d)) / 4
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    return s, t, perm.astype(np.int64)
