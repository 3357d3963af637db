"""Seeded cases of the supervised classification tests.

Golden cases (tests/golden/classification_<name>.npz, written by
tests/golden/make_classification_goldens.py): a model scikit-learn trained on
``training_set(spec)`` and what it predicts for ``table(spec)``.  Constructed
cases: forests built by hand, with the literal as the expectation.
"""
import numpy as np

#: name -> spec.  n: rows predicted; n_train: rows trained on.
FOREST_GOLDEN = {
    # 3 depth-3 trees, more than one workgroup of rows (1,024 rows each)
    "forest_d7_c5_t3": dict(n=2100, d=7, classes=5, trees=3, depth=3, n_train=400, seed=11, spread=3.0),
    # the reference's largest search point: 24 unlimited-depth trees
    "forest_d33_c2_t24": dict(n=400, d=33, classes=2, trees=24, depth=None, n_train=600, seed=12,
                              spread=8.0),
    # one feature, 16 classes, one tree that is a single leaf
    "forest_d1_c16_leaf": dict(n=700, d=1, classes=16, trees=5, depth=6, n_train=480, seed=13,
                               spread=1.0, single_leaf_at=2),
    # the widest table
    "forest_d256_c2_t6": dict(n=40, d=256, classes=2, trees=6, depth=None, n_train=200, seed=14,
                              spread=16.0),
}

SVC_GOLDEN = {
    # more than one workgroup of rows; rows one below, at and above the row tile
    "svc_rbf_d7_k3": dict(n=1300, d=7, classes=3, kernel="rbf", C=8.0, gamma=2.0 ** -3,
                          n_train=300, seed=21, scaler=True),
    # a hard margin: large coefficients
    "svc_rbf_d33_k5": dict(n=300, d=33, classes=5, kernel="rbf", C=2.0 ** 15, gamma=2.0 ** -7,
                           n_train=400, seed=22, scaler=True),
    "svc_rbf_d1_k2": dict(n=500, d=1, classes=2, kernel="rbf", C=8.0, gamma=2.0 ** -3,
                          n_train=120, seed=23, scaler=False),
    "svc_rbf_d5_k16": dict(n=80, d=5, classes=16, kernel="rbf", C=8.0, gamma=2.0 ** -3,
                           n_train=480, seed=24, scaler=True),
    "svc_linear_d7_k5": dict(n=700, d=7, classes=5, kernel="linear", C=1.0, gamma=2.0 ** -3,
                             n_train=300, seed=25, scaler=True),
    "svc_linear_d256_k2": dict(n=40, d=256, classes=2, kernel="linear", C=1.0, gamma=2.0 ** -3,
                               n_train=120, seed=26, scaler=False),
}


def _blobs(rs, n, d, classes, spread):
    """class centres on a seeded lattice, rows around them; values are multiples
    of 1/256, so that the stored tables compress"""
    centres = rs.uniform(-4.0, 4.0, size=(classes, d))
    y = np.arange(n) % classes
    rs.shuffle(y)
    X = centres[y] + rs.normal(0.0, spread, size=(n, d))
    return np.round(X * 256.0) / 256.0, y


def training_set(spec):
    rs = np.random.RandomState(spec["seed"])
    X, y = _blobs(rs, spec["n_train"], spec["d"], spec["classes"], spec.get("spread", 1.5))
    # labels as the tool hands them over: floats 0.0, 1.0, ...
    return 100.0 * X + 3.0 if spec.get("scaler") else X, y.astype(np.float64)


def table(spec):
    """the rows to predict: the training distribution, wider, from another seed"""
    rs = np.random.RandomState(spec["seed"])
    centres = rs.uniform(-4.0, 4.0, size=(spec["classes"], spec["d"]))
    rs = np.random.RandomState(spec["seed"] + 1000)
    y = rs.randint(spec["classes"], size=spec["n"])
    X = np.round((centres[y] + rs.normal(0.0, 2.5, size=(spec["n"], spec["d"]))) * 256.0) / 256.0
    return 100.0 * X + 3.0 if spec.get("scaler") else X


# ---- forests built by hand ----------------------------------------------------------

def leaf(*fractions):
    return ("leaf", [float(v) for v in fractions])


def node(feature, threshold, left, right):
    return ("node", int(feature), float(threshold), left, right)


def forest_model(trees, d, n_classes):
    """The flat model of nested ``node`` / ``leaf`` trees, every tree numbered
    breadth first: children lie after their parent but not next to it."""
    feature, threshold, left, right, leaf_row, values, roots = [], [], [], [], [], [], []
    for tree in trees:
        base = len(feature)
        roots.append(base)
        queue = [tree]
        at = 0
        while at < len(queue):
            t = queue[at]
            at += 1
            if t[0] == "leaf":
                feature.append(-1)
                threshold.append(0.0)
                left.append(0)
                right.append(0)
                leaf_row.append(len(values))
                values.append(t[1])
                continue
            feature.append(t[1])
            threshold.append(t[2])
            left.append(base + len(queue))
            right.append(base + len(queue) + 1)
            leaf_row.append(0)
            queue += [t[3], t[4]]
    return {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float64),
            "left": np.array(left, np.int32), "right": np.array(right, np.int32),
            "tree_root": np.array(roots, np.int32), "leaf_row": np.array(leaf_row, np.int32),
            "leaf_value": np.array(values, np.float64).reshape(-1, n_classes),
            "n_features": np.int64(d), "classes": np.arange(n_classes, dtype=np.float64)}


#: a threshold that is a float32 value, and the float64 just above it: the
#: float64 compares greater, its float32 cast equal
F32_THRESHOLD = float(np.float32(1.1))
JUST_ABOVE = float(np.nextafter(np.float64(F32_THRESHOLD), np.inf))


def threshold_case():
    """rows that equal a threshold exactly, and rows whose f64 value lies just
    above a threshold while their f32 cast does not"""
    model = forest_model([node(0, F32_THRESHOLD, leaf(1, 0), leaf(0, 1)),
                          node(1, -2.5, leaf(1, 0), node(0, 0.5, leaf(0.25, 0.75), leaf(0, 1)))],
                         2, 2)
    X = np.array([[F32_THRESHOLD, -2.5],        # both equal: left, left
                  [JUST_ABOVE, -2.5],           # f64 above, f32 equal: left
                  [JUST_ABOVE, 0.0],
                  [np.nextafter(np.float64(F32_THRESHOLD), -np.inf), 3.0],
                  [float(np.nextafter(np.float32(1.1), np.float32(2.0))), 3.0],   # the next f32: right
                  [0.5, 0.0],                   # the inner threshold, equal: left
                  [np.nextafter(0.5, 1.0), 0.0],    # rounds to 0.5 in f32: left
                  [-1.0, -3.0]], dtype=np.float64)
    return model, X


def tie_case():
    """two trees that disagree with pure leaves: the exact tie goes to the first class"""
    model = forest_model([leaf(0, 1, 0), leaf(1, 0, 0)], 1, 3)
    return model, np.array([[-1.0], [0.0], [2.0]])


def divide_case():
    """Three single-leaf trees whose class sums a < b are neighbouring doubles in
    [1.5, 2) with a / 3 == b / 3: dropping the divide labels the rows 1, the
    rule labels them 0.  (a / 3 lies in [0.5, 2/3), where doubles are 2^-53
    apart while the quotients of neighbours are 2^-52 / 3 apart.)"""
    a = np.float64(1.5)
    while True:
        b = np.nextafter(a, 2.0)
        if a / 3.0 == b / 3.0:
            break
        a = b
    model = forest_model([leaf(a, b), leaf(0, 0), leaf(0, 0)], 1, 2)
    return model, np.array([[0.0], [1.0]]), float(a), float(b)


def big_forest(seed=5, trees=8, depth=10, d=5, n_classes=4):
    """complete trees of the given depth: 8 * 2,047 nodes, beyond the LDS route"""
    rs = np.random.RandomState(seed)

    def grow(level):
        if level == depth:
            p = rs.randint(0, 8, size=n_classes).astype(np.float64)
            p[rs.randint(n_classes)] += 1.0
            return leaf(*(p / p.sum()))
        return node(rs.randint(d), np.round(rs.normal(0.0, 1.5) * 64.0) / 64.0, grow(level + 1),
                    grow(level + 1))

    model = forest_model([grow(0) for _ in range(trees)], d, n_classes)
    X = np.round(rs.normal(0.0, 2.0, size=(300, d)) * 64.0) / 64.0   # thresholds are hit exactly
    return model, X


def small_forest():
    """a sound model to break one way at a time"""
    return forest_model([node(1, 0.5, node(0, -1.0, leaf(1, 0), leaf(0.5, 0.5)), leaf(0, 1)),
                         node(2, 0.0, leaf(0.25, 0.75), leaf(1, 0))], 3, 2)


def malformed_forests():
    """name -> model that ``tmh_forest_create`` must refuse"""
    out = {}

    def broken(name, **changes):
        m = {k: np.array(v, copy=True) for k, v in small_forest().items()}
        for key, (index, value) in changes.items():
            m[key][index] = value
        out[name] = m

    broken("child_equals_parent", left=(0, 0))
    broken("child_below_parent", right=(1, 0))
    broken("child_in_next_tree", right=(0, 5))
    broken("child_past_the_end", left=(5, 8))
    broken("feature_at_d", feature=(1, 3))
    broken("feature_negative", feature=(0, -2))
    broken("threshold_nan", threshold=(5, np.nan))
    broken("leaf_row_out_of_range", leaf_row=(2, 5))
    broken("leaf_value_infinite", leaf_value=((0, 1), np.inf))
    broken("first_root_not_zero", tree_root=(0, 1))
    broken("node_reached_twice", left=(0, 2))       # node 2 is node 0's right child too
    return out


def small_svc(kernel="rbf"):
    """a sound SVC model: 3 classes, 2 features, 5 support vectors"""
    return {"kernel": np.str_(kernel), "gamma": np.float64(0.5),
            "sv": np.array([[0.0, 0.0], [1.0, 0.5], [2.0, 2.0], [-1.0, 1.0], [0.5, -2.0]]),
            "n_sv": np.array([2, 1, 2], np.int32),
            "coef": np.array([[0.5, 1.0, -1.5, -0.25, -0.75], [0.25, 0.5, 1.0, -1.0, -0.5]]),
            "rho": np.array([0.1, -0.2, 0.05]), "classes": np.arange(3, dtype=np.float64)}
