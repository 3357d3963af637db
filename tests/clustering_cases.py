"""Inputs of the clustering tests, each from a fixed seed (legacy RandomState:
the same bytes on every numpy).  A case is raw features X [n][d] and, for the
k-means cases, initial centres C0 [k][d] in the SCALED space; the scaler is
always RobustScaler(quantile_range=(1, 99)) fitted on X.
"""
import numpy as np

import clustering_literal as lit

#: the assign kernel's row tile at d = 20 (2,048 staged values per tile, even);
#: a workgroup owns a chunk of 1,024 rows and its tiles start at the chunk's
#: first row, so the second chunk's tiles end at rows 1,024 + 102 m
TILE_D = 20
TILE_ROWS = 102
CHUNK_ROWS = 1024

#: name -> (n, d, k, seed, kind)
KMEANS_CASES = {
    "n4097_d3_k2": (4097, 3, 2, 11, "gauss"),
    "n3001_d33_k9": (3001, 33, 9, 12, "gauss_const"),   # column 5 is constant: zero scale
    "n5000_d7_k4_blobs": (5000, 7, 4, 13, "blobs"),
    "n257_d1_k1": (257, 1, 1, 14, "gauss"),
    "n2048_d128_k64": (2048, 128, 64, 15, "gauss"),     # the k limit
    "n1000_d256_k32": (1000, 256, 32, 16, "gauss"),     # the d limit, k * d = 8,192
    "tile_below": (CHUNK_ROWS + TILE_ROWS * 3 - 1, TILE_D, 8, 17, "blobs"),   # last tile: 101 rows
    "tile_above": (CHUNK_ROWS + TILE_ROWS * 3 + 1, TILE_D, 8, 18, "blobs"),   # last tile: 1 row
    "one_empty": (5000, 7, 4, 19, "blobs_empty1"),
    "two_empty": (5000, 7, 5, 20, "blobs_empty2"),
}
#: compared with scikit-learn's recorded results (two_empty: the literal alone,
#: scikit-learn leaves the order inside its top set open)
GOLDEN_CASES = [c for c in KMEANS_CASES if c != "two_empty"]

SCALER_ONLY_CASES = ("nan_column", "zeros_and_duplicates")


def _features(rs, n, d, kind, k):
    if kind.startswith("blobs"):
        groups = max(k, 2)
        centres = rs.uniform(-20.0, 20.0, size=(groups, d))
        member = rs.randint(groups, size=n)
        X = centres[member] + rs.normal(size=(n, d))
    else:
        X = rs.normal(size=(n, d)) * rs.uniform(0.5, 50.0, size=d) + rs.uniform(-100.0, 100.0, size=d)
    if kind == "gauss_const":
        X[:, 5] = 3.25
    return np.ascontiguousarray(X)


def kmeans_case(name):
    """-> dict: X, center, scale, Xs (the scaled table), C0, k"""
    n, d, k, seed, kind = KMEANS_CASES[name]
    rs = np.random.RandomState(seed)
    X = _features(rs, n, d, kind, k)
    center, scale = lit.robust_fit(X)
    Xs = lit.robust_transform(X, center, scale)
    C0 = Xs[rs.choice(n, size=k, replace=False)].copy()
    if kind == "blobs_empty1":
        C0[2] = 1000.0          # far outside the data: empty at the first iteration
    if kind == "blobs_empty2":
        C0[1] = 1000.0
        C0[3] = -1000.0
    return {"X": X, "center": center, "scale": scale, "Xs": Xs, "C0": C0, "k": k}


def scaler_case(name):
    """raw X of the scaler-only cases"""
    if name == "nan_column":
        rs = np.random.RandomState(31)
        X = rs.normal(size=(3001, 5)) * 7.0
        X[rs.choice(3001, size=300, replace=False), 2] = np.nan
        return np.ascontiguousarray(X)
    if name == "zeros_and_duplicates":
        rs = np.random.RandomState(32)
        n = 1000
        X = rs.normal(size=(n, 3))
        # sorted: 5 x -2, 20 x -1 (the 1 % ranks 9, 10), 950 zeros of both signs
        # (the middle ranks 499, 500), 25 x 3 (the 99 % ranks 989, 990)
        zeros = np.where(rs.randint(2, size=950) == 0, -0.0, 0.0)
        col = np.concatenate([np.full(5, -2.0), np.full(20, -1.0), zeros, np.full(25, 3.0)])
        X[:, 1] = col[rs.permutation(n)]
        return np.ascontiguousarray(X)
    raise KeyError(name)


def all_scaler_inputs():
    """name -> raw X of every case the scaler is checked on"""
    out = {name: kmeans_case(name)["X"] for name in KMEANS_CASES}
    for name in SCALER_ONLY_CASES:
        out[name] = scaler_case(name)
    return out
