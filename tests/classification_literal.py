"""The supervised classification tool's two prediction rules in plain numpy
(DESIGN.md section 23), as scikit-learn 1.7.2 runs them.

Forest (``RandomForestClassifier.predict`` with ``n_jobs=1``): X is cast to
float32; at a node the row goes left iff ``float64(x_f32[feature]) <=
threshold``; a leaf contributes its row of fractions; the trees' rows are added
in f64 in tree order into zero; each class sum is divided by ``n_trees`` once;
the label is the first maximum.

SVC (libsvm's dense ``svm_predict_values``): ``K = exp(-gamma sum (x - sv)^2)``
or ``x . sv``; for each class pair (i < j) in libsvm's order
``dec = sum_{SVs of i} coef[j - 1][s] K_s + sum_{SVs of j} coef[i][s] K_s -
rho[p]``; the vote goes to i iff ``dec > 0``; the label is the first class with
the most votes.  A row is *close* when some pair has
``|dec| <= 64 (d + m_pair) 2^-52 (sum_s |coef_s| A_s + |rho|)``, ``A_s = 1`` for
rbf and ``sum_f |x_f sv_sf|`` for linear: there the summation order, which is
free, may decide the vote.
"""
import numpy as np

EPS = 2.0 ** -52
F32_MAX = float(np.finfo(np.float32).max)


def forest_arrays(model):
    return (model["feature"], model["threshold"], model["left"], model["right"],
            model["tree_root"], model["leaf_row"], model["leaf_value"])


def forest_validate(model):
    """None, or why ``tmh_forest_create`` refuses the model (the same checks in
    the same order as classify_core.h's forest_validate and forest_pack)."""
    feature, threshold, left, right, roots, leaf_row, value = forest_arrays(model)
    nodes, d = feature.size, int(model["n_features"])
    n_leaves, n_classes = value.shape
    if not 1 <= d <= 256:
        return "d"
    if not 2 <= n_classes <= 64:
        return "n_classes"
    if not 1 <= roots.size <= 256:
        return "n_trees"
    if not 1 <= nodes < 2 ** 24:
        return "nodes"
    if not 1 <= n_leaves <= nodes:
        return "n_leaves"
    if roots[0] != 0:
        return "first root"
    seen = np.zeros(nodes, bool)
    for t in range(roots.size):
        lo = int(roots[t])
        hi = int(roots[t + 1]) if t + 1 < roots.size else nodes
        if lo < 0 or lo >= hi or hi > nodes:
            return "roots"
        for i in range(lo, hi):
            if feature[i] == -1:
                if not 0 <= leaf_row[i] < n_leaves:
                    return "leaf row"
                continue
            if not 0 <= feature[i] < d:
                return "feature"
            if np.isnan(threshold[i]):
                return "threshold"
            if not (lo <= left[i] < hi and lo <= right[i] < hi):
                return "outside"
            if left[i] <= i or right[i] <= i:
                return "order"
    if not np.isfinite(value).all():
        return "leaf value"
    for t in range(roots.size):
        stack = [int(roots[t])]
        while stack:
            i = stack.pop()
            if seen[i]:
                return "twice"
            seen[i] = True
            if feature[i] != -1:
                stack += [int(right[i]), int(left[i])]
    return None


def forest_leaves(model, X):
    """leaf_value row [n][n_trees] every row ends in, walking node by node"""
    feature, threshold, left, right, roots, leaf_row, _ = forest_arrays(model)
    Xf = np.asarray(X, np.float64).astype(np.float32)
    out = np.zeros((Xf.shape[0], roots.size), dtype=np.int64)
    for r in range(Xf.shape[0]):
        for t in range(roots.size):
            i = int(roots[t])
            while feature[i] != -1:
                i = int(left[i]) if np.float64(Xf[r, feature[i]]) <= threshold[i] else int(right[i])
            out[r, t] = leaf_row[i]
    return out


def forest_predict(model, X):
    """-> (labels [n] as indices into classes, proba [n][n_classes])"""
    value = model["leaf_value"]
    leaves = forest_leaves(model, X)
    proba = np.zeros((leaves.shape[0], value.shape[1]), dtype=np.float64)
    for t in range(leaves.shape[1]):
        proba += value[leaves[:, t]]
    proba /= leaves.shape[1]
    return np.argmax(proba, axis=1), proba


def forest_refuses(X):
    """what the forest refuses: NaN, +-inf, or a finite value whose f32 cast is infinite"""
    X = np.asarray(X, np.float64)
    with np.errstate(over="ignore"):
        return bool(not np.isfinite(X).all() or not np.isfinite(X.astype(np.float32)).all())


def svc_pairs(k):
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def svc_predict(model, Xs):
    """-> (labels [n] as indices into classes, dec [n][pairs], close [n]) for the
    scaled table Xs"""
    Xs = np.asarray(Xs, np.float64)
    sv, n_sv, coef, rho = model["sv"], model["n_sv"], model["coef"], model["rho"]
    kernel, gamma = str(model["kernel"]), float(model["gamma"])
    n, d = Xs.shape
    k = n_sv.size
    start = np.concatenate([[0], np.cumsum(n_sv)]).astype(np.int64)
    if kernel == "rbf":
        K = np.empty((n, sv.shape[0]))
        for s in range(sv.shape[0]):
            diff = Xs - sv[s]
            K[:, s] = np.exp(-gamma * (diff * diff).sum(axis=1))
        A = np.ones_like(K)
    else:
        K = Xs @ sv.T
        A = np.abs(Xs) @ np.abs(sv).T
    pairs = svc_pairs(k)
    dec = np.empty((n, len(pairs)))
    close = np.zeros(n, bool)
    votes = np.zeros((n, k), dtype=np.int64)
    for p, (i, j) in enumerate(pairs):
        si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
        ci, cj = coef[j - 1, si], coef[i, sj]
        dec[:, p] = K[:, si] @ ci + K[:, sj] @ cj - rho[p]
        mag = A[:, si] @ np.abs(ci) + A[:, sj] @ np.abs(cj) + abs(rho[p])
        m_pair = int(n_sv[i] + n_sv[j])
        close |= np.abs(dec[:, p]) <= 64 * (d + m_pair) * EPS * mag
        votes[:, i] += dec[:, p] > 0
        votes[:, j] += ~(dec[:, p] > 0)
    return np.argmax(votes, axis=1), dec, close


def svc_dec_bound(model, Xs):
    """[n][pairs]: the close-row rule's bound, which is also the decision values' tolerance"""
    Xs = np.asarray(Xs, np.float64)
    sv, n_sv, coef, rho = model["sv"], model["n_sv"], model["coef"], model["rho"]
    d = Xs.shape[1]
    start = np.concatenate([[0], np.cumsum(n_sv)]).astype(np.int64)
    if str(model["kernel"]) == "rbf":
        A = np.ones((Xs.shape[0], sv.shape[0]))
    else:
        A = np.abs(Xs) @ np.abs(sv).T
    out = []
    for p, (i, j) in enumerate(svc_pairs(n_sv.size)):
        si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
        mag = A[:, si] @ np.abs(coef[j - 1, si]) + A[:, sj] @ np.abs(coef[i, sj]) + abs(rho[p])
        out.append(64 * (d + int(n_sv[i] + n_sv[j])) * EPS * mag)
    return np.stack(out, axis=1)


def scale(X, center, scale_):
    return (np.asarray(X, np.float64) - center) / scale_
