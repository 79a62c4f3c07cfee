"""numpy restatements of the four metrics the Minkowski-family VALU path computes beyond the Minkowski family itself:
braycurtis, seuclidean, correlation and hamming.

They are the specification the device follows (kz_common.h: kz_family_term / kz_family_add, kz_exact.h: kz_family_dist_kernel):
each function evaluates ONE expression per pair, vectorised over all pairs of a query block and an index block, with the loop over
features written out so that the order of the additions is the order the kernels use.  tests/test_metrics_extra.py checks them
against scikit-learn bit for bit; the GPU tests check the device against scikit-learn through them.

  braycurtis   sklearn DistanceMetric{32,64} (BrayCurtisDistance): num += |x_j - y_j|, den += |x_j| + |y_j| (the difference in the
               input dtype, everything else float64); num / den, 0 where den == 0; rounded to float32 for float32 inputs.
  seuclidean   SEuclideanDistance: t = x_j - y_j in the input dtype, s += t t / V_j (a true division); ranking value s (rounded to
               float32 for float32 inputs), distance sqrt(s) (rounded to float32 for float32 inputs).
  correlation  scipy.spatial.distance.cdist: rows in float64, u = x - mean(x) (numpy's pairwise mean), a dot product in two
               interleaved partial sums (even / odd features, then the odd tail term), c = u.v / (|u| |v|) with |u| = sqrt(u.u),
               |c| > 1 clipped to +-1, value 1 - c (NaN for a constant row).
  hamming      cdist: count(x_j != y_j) / d, float64.
"""
import numpy as np

EXTRA_METRICS = ("braycurtis", "seuclidean", "correlation", "hamming")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def braycurtis_values(x, y):
    """[n_x, n_y] ranking values (= distances)."""
    x, y = np.asarray(x), np.asarray(y)
    num = np.zeros((x.shape[0], y.shape[0]))
    den = np.zeros((x.shape[0], y.shape[0]))
    for j in range(x.shape[1]):
        xj, yj = x[:, None, j], y[None, :, j]
        num += np.abs(xj - yj).astype(np.float64)                    # (difference in the input dtype)
        den += np.abs(xj).astype(np.float64) + np.abs(yj).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
    return v.astype(np.float32).astype(np.float64) if x.dtype == np.float32 else v


def seuclidean_values(x, y, V):
    """[n_x, n_y] ranking values s (the distance is seuclidean_distance(s, dtype))."""
    x, y, V = np.asarray(x), np.asarray(y), _f64(V)
    s = np.zeros((x.shape[0], y.shape[0]))
    for j in range(x.shape[1]):
        t = (x[:, None, j] - y[None, :, j]).astype(np.float64)
        s += t * t / V[j]
    return s.astype(np.float32).astype(np.float64) if x.dtype == np.float32 else s


def seuclidean_distance(s, dtype):
    d = np.sqrt(s)
    return d.astype(np.float32).astype(np.float64) if np.dtype(dtype) == np.float32 else d


def _dot2(a, b):
    """scipy's dot product of the (broadcast) rows a, b: even features into s0, odd ones into s1, s0 + s1, then the odd tail."""
    d = a.shape[-1]
    s0 = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]))
    s1 = np.zeros_like(s0)
    for j in range(0, d - 1, 2):
        s0 += a[..., j] * b[..., j]
        s1 += a[..., j + 1] * b[..., j + 1]
    s = s0 + s1
    if d % 2:
        s += a[..., d - 1] * b[..., d - 1]
    return s


def correlation_centre(x):
    """(centred float64 rows, their norms sqrt(u.u)): the per-row state the device keeps (kz_pack.hip: the correlation rows)."""
    x = _f64(x)
    u = x - x.mean(axis=1, keepdims=True)     # numpy's pairwise sum per row, / d
    return u, np.sqrt(_dot2(u, u))


def correlation_values(x, y):
    u, nu = correlation_centre(x)
    v, nv = correlation_centre(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = _dot2(u[:, None, :], v[None, :, :]) / (nu[:, None] * nv[None, :])
    big = np.abs(c) > 1.0
    c[big] = np.copysign(1.0, c[big])
    return 1.0 - c


def hamming_values(x, y):
    x, y = np.asarray(x), np.asarray(y)
    cnt = np.zeros((x.shape[0], y.shape[0]))
    for j in range(x.shape[1]):
        cnt += (x[:, None, j] != y[None, :, j])
    return cnt / x.shape[1]


def ranking_values(metric, x, y, V=None):
    if metric == "braycurtis":
        return braycurtis_values(x, y)
    if metric == "seuclidean":
        return seuclidean_values(x, y, V)
    if metric == "correlation":
        return correlation_values(x, y)
    if metric == "hamming":
        return hamming_values(x, y)
    raise ValueError(metric)


def output_distance(metric, vals, dtype):
    return seuclidean_distance(vals, dtype) if metric == "seuclidean" else vals


def knn(metric, x, y, k, V=None, exclude_self=False):
    """(dist, ind) of the k nearest rows of y for every row of x, by (ranking value, index row), NaN after every finite value;
    exclude_self: scikit-learn's self removal (sklearn/neighbors/_base.py: the query row dropped among the first k + 1)."""
    vals = ranking_values(metric, x, y, V)
    kk = k + 1 if exclude_self else k
    # (NaN ranks as +inf, which none of the four metrics reaches otherwise; ties by index row)
    order = np.argsort(np.where(np.isnan(vals), np.inf, vals), axis=1, kind="stable")[:, :kk]
    if exclude_self:
        out = np.empty((x.shape[0], k), dtype=np.int64)
        for r in range(x.shape[0]):
            row = list(order[r])
            row.remove(r) if r in row else row.pop(0)
            out[r] = row[:k]
        order = out
    dist = np.take_along_axis(vals, order, axis=1)
    return output_distance(metric, dist, np.asarray(x).dtype), order.astype(np.int64)
