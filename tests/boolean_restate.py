"""numpy restatement of scipy's seven boolean metrics as the device computes them (kiez_amd/csrc/kz_bool.h: kz_bool_finish).

scikit-learn sends these names through pairwise_distances: the rows cast to bool (x != 0, so -0.0 is false) and handed to
scipy.spatial.distance.cdist; the result is float64 whatever the input dtype.  A pair's value is a function of four integers.  With
n = d, nx / ny the rows' numbers of true features and ntt = popcount(x & y):

    ndf = nx + ny - 2 ntt      ntf = nx - ntt      nft = ny - ntt      nff = n - ntt - ndf

every integer is converted exactly to float64 and each value takes ONE division:

    jaccard                          0 if ntt + ndf == 0, else ndf / (ntt + ndf)
    dice                             ndf / (2 ntt + ndf)                      (0 / 0 -> NaN: two all-false rows)
    rogerstanimoto, sokalmichener    2 ndf / (n + ndf)
    russellrao                       (n - ntt) / n
    sokalsneath                      2 ndf / (2 ndf + ntt)                    (0 / 0 -> NaN: two all-false rows)
    yule                             h = ntf nft; 0 if h == 0, else 2 h / (ntt nff + h)

tests/test_boolean_metrics.py checks these against scikit-learn bit for bit; the GPU tests check the device through them.
"""
import numpy as np

BOOLEAN_METRICS = ("jaccard", "dice", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "yule")


def counts(x, y):
    """(ntt [n_x, n_y], nx [n_x, 1], ny [1, n_y], n) as float64 (exact: every count is an integer below 2^26)."""
    xb, yb = (np.asarray(x) != 0), (np.asarray(y) != 0)
    ntt = xb.astype(np.float64) @ yb.astype(np.float64).T          # (sums of 0 / 1 products: exact in any order)
    return ntt, xb.sum(axis=1, dtype=np.int64).astype(np.float64)[:, None], yb.sum(axis=1, dtype=np.int64).astype(np.float64)[None, :], \
        float(xb.shape[1])


def ranking_values(metric, x, y):
    """[n_x, n_y] float64 values (= the distances returned), NaN where scipy has NaN."""
    ntt, nx, ny, n = counts(x, y)
    ndf = nx + ny - 2.0 * ntt
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "jaccard":
            den = ntt + ndf
            return np.where(den == 0, 0.0, ndf / np.where(den == 0, 1.0, den))
        if metric == "dice":
            return ndf / (2.0 * ntt + ndf)
        if metric in ("rogerstanimoto", "sokalmichener"):
            return (2.0 * ndf) / (n + ndf)
        if metric == "russellrao":
            return (n - ntt) / n
        if metric == "sokalsneath":
            return (2.0 * ndf) / (2.0 * ndf + ntt)
        if metric == "yule":
            h = (nx - ntt) * (ny - ntt)
            nff = n - ntt - ndf
            den = ntt * nff + h
            return np.where(h == 0, 0.0, (2.0 * h) / np.where(h == 0, 1.0, den))
    raise ValueError(metric)


def knn(metric, x, y, k, exclude_self=False):
    """(dist, ind) of the k nearest rows of y for every row of x by (value, index row), NaN after every finite value (ranked as +inf,
    which none of the seven metrics reaches otherwise); exclude_self: scikit-learn's self removal (the query row dropped among the
    first k + 1, else the first entry)."""
    vals = ranking_values(metric, x, y)
    kk = k + 1 if exclude_self else k
    order = np.argsort(np.where(np.isnan(vals), np.inf, vals), axis=1, kind="stable")[:, :kk]
    if exclude_self:
        out = np.empty((vals.shape[0], k), dtype=np.int64)
        for r in range(vals.shape[0]):
            row = list(order[r])
            row.remove(r) if r in row else row.pop(0)
            out[r] = row[:k]
        order = out
    return np.take_along_axis(vals, order, axis=1), order.astype(np.int64)
