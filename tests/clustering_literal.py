"""Plain numpy restatement of the clustering tool's rules (the tests' literal).

RobustScaler(quantile_range=(lo, hi)): per column over its non-NaN values,
``center_`` is the median -- (a + b) / 2 of the two middle order statistics --
and ``scale_`` the difference of numpy's 'linear' percentiles, a zero scale
becoming 1.  KMeans: scikit-learn's ``_kmeans_single_lloyd`` with
``_relocate_empty_clusters_dense`` (the order inside the top set fixed: rows in
descending distance, ties to the lowest row) and ``_kmeans_plusplus`` from
given draws.
"""
import numpy as np

EPS = 2.0 ** -52


# ---- scaler ---------------------------------------------------------------------

def percentile_ranks(m, q_percent):
    """(lo, hi, gamma) of numpy's 'linear' percentile over m sorted values."""
    v = (m - 1) * (np.float64(q_percent) / 100.0)
    lo = int(np.floor(v))
    hi = min(lo + 1, m - 1)
    return lo, hi, v - lo


def lerp(a, b, t):
    """numpy's _lerp for scalars"""
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def column_ranks(m, quantile_range=(1.0, 99.0)):
    """The six 0-based ranks a column of m values needs: the two middle values,
    then (lo, hi) of each percentile; and the two lerp weights."""
    l0, h0, g0 = percentile_ranks(m, quantile_range[0])
    l1, h1, g1 = percentile_ranks(m, quantile_range[1])
    return [(m - 1) // 2, m // 2, l0, h0, l1, h1], (g0, g1)


def finish_column(values, gammas):
    """center and scale of a column from its six order statistics"""
    a, b, p0, p1, p2, p3 = values
    center = (a + b) / 2
    scale = lerp(p2, p3, gammas[1]) - lerp(p0, p1, gammas[0])
    return center, (1.0 if scale == 0.0 else scale)


def robust_fit(X, quantile_range=(1.0, 99.0)):
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    center, scale = np.empty(d), np.empty(d)
    for f in range(d):
        col = X[:, f]
        s = np.sort(col[~np.isnan(col)])
        ranks, gammas = column_ranks(s.size, quantile_range)
        center[f], scale[f] = finish_column([s[r] for r in ranks], gammas)
    return center, scale


def robust_transform(X, center, scale):
    return (np.asarray(X, dtype=np.float64) - center) / scale


# ---- Lloyd ------------------------------------------------------------------------

def sq_distances(X, C):
    """[n][k] direct differenced squared distances"""
    out = np.empty((X.shape[0], C.shape[0]))
    for j in range(C.shape[0]):
        diff = X - C[j]
        out[:, j] = (diff * diff).sum(axis=1)
    return out


def close_rows(D, d):
    """rows whose two smallest squared distances differ by less than
    64 d 2^-52 of their sum"""
    if D.shape[1] < 2:
        return np.zeros(D.shape[0], dtype=bool)
    part = np.partition(D, 1, axis=1)
    a, b = part[:, 0], part[:, 1]
    return (b - a) < 64 * d * EPS * (a + b)


def assign(X, C):
    D = sq_distances(X, C)
    labels = np.argmin(D, axis=1)
    return labels, D[np.arange(X.shape[0]), labels], D


def update(X, labels, mind, C_old):
    k, d = C_old.shape
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, d))
    for j in range(k):
        sums[j] = X[labels == j].sum(axis=0)
    empty = np.flatnonzero(counts == 0)
    if empty.size:
        # descending distance, ties to the lowest row
        order = np.lexsort((np.arange(X.shape[0]), -mind))
        for e, row in zip(empty, order[:empty.size]):
            old = labels[row]
            sums[old] -= X[row]
            sums[e] = X[row]
            counts[old] -= 1
            counts[e] = 1
    C_new = C_old.copy()
    has = counts > 0
    C_new[has] = sums[has] / counts[has, None]
    return C_new


def tolerance(X, tol):
    return float(np.mean(np.var(X, axis=0)) * tol)


def lloyd(X, C0, max_iter=300, tol=1e-4, history=None):
    """-> labels, centres, inertia, n_iter, tol_abs.  history (a list): per
    iteration (centres used, centre shift) and per assign the distance table's
    close rows are appended by the callers that want them."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    tol_abs = tolerance(X, tol)
    prev = np.full(X.shape[0], -1)
    strict = False
    n_iter = 0
    for i in range(max_iter):
        labels, mind, D = assign(X, C)
        C_new = update(X, labels, mind, C)
        shift = float(((C_new - C) ** 2).sum())
        if history is not None:
            history.append({"centres": C.copy(), "shift": shift,
                            "close": int(close_rows(D, X.shape[1]).sum())})
        C = C_new
        n_iter = i + 1
        if np.array_equal(labels, prev):
            strict = True
            break
        if shift <= tol_abs:
            break
        prev = labels
    if not strict:
        labels, mind, D = assign(X, C)
        if history is not None:
            history.append({"centres": C.copy(), "shift": None,
                            "close": int(close_rows(D, X.shape[1]).sum())})
    return labels, C, float(mind.sum()), n_iter, tol_abs


# ---- seeding ------------------------------------------------------------------------

def n_local_trials(k):
    return 2 + int(np.log(k))


def seed_draws(rs, n, k):
    """first index and draws [k - 1][trials] from a RandomState, in call order"""
    first = int(rs.randint(n))
    trials = n_local_trials(k)
    draws = np.empty((k - 1, trials))
    for c in range(k - 1):
        draws[c] = rs.uniform(size=trials)
    return first, draws


def kmeans_plusplus(X, k, first, draws):
    """-> indices [k], per-step trace: targets, cumsum, candidates, pots, kept, pot"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    indices = [int(first)]
    diff = X - X[first]
    closest = (diff * diff).sum(axis=1)
    pot = float(closest.sum())
    trace = []
    for c in range(1, k):
        targets = draws[c - 1] * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, targets), n - 1)
        trial = np.empty((cand.size, n))
        for t, row in enumerate(cand):
            diff = X - X[row]
            trial[t] = np.minimum(closest, (diff * diff).sum(axis=1))
        pots = trial.sum(axis=1)
        best = int(np.argmin(pots))
        trace.append({"targets": targets, "cumsum": cum, "closest": closest, "cand": cand,
                      "pots": pots, "best": best, "pot": pot})
        pot = float(pots[best])
        closest = trial[best]
        indices.append(int(cand[best]))
    return np.array(indices), trace
