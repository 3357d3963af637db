"""Writes tests/golden/clustering_<case>.npz: what scikit-learn computes for the
cases of tests/clustering_cases.py.

    python tests/golden/make_clustering_goldens.py

Per case: RobustScaler(quantile_range=(1, 99)).center_ / scale_; for the
k-means cases the labels (uint8), centres, inertia and n_iter_ of
KMeans(init=C0, n_init=1, algorithm='lloyd') on the scaled table, at tol=0
(`t0_*`) and at the default tol (`td_*`), and the literal's tol_abs.

The generator asserts what the tests rely on and fails otherwise:
  * the literal (tests/clustering_literal.py) reproduces scikit-learn: scaler
    bit for bit, labels without a mismatch, n_iter_ exactly;
  * the literal meets no close row (clustering_literal.close_rows) at any
    iteration of any case;
  * at the default tol no centre shift lies within 1e-6 relative of tol_abs;
  * in the one-empty case the farthest row is unique.
"""
import os
import sys

import numpy as np
from sklearn.cluster import KMeans
from sklearn.preprocessing import RobustScaler

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import clustering_cases as cases  # noqa: E402
import clustering_literal as lit  # noqa: E402


def scaler_golden(X):
    sk = RobustScaler(quantile_range=(1.0, 99.0)).fit(X)
    center, scale = lit.robust_fit(X)
    assert np.array_equal(sk.center_, center), "center_ differs from the literal"
    assert np.array_equal(sk.scale_, scale), "scale_ differs from the literal"
    ok = ~np.isnan(X)
    assert np.array_equal(sk.transform(X)[ok], lit.robust_transform(X, center, scale)[ok])
    return {"center": sk.center_, "scale": sk.scale_}


def kmeans_golden(name, case, tol, prefix):
    Xs, C0, k = case["Xs"], case["C0"], case["k"]
    sk = KMeans(n_clusters=k, init=C0, n_init=1, algorithm="lloyd", tol=tol).fit(Xs)
    history = []
    labels, C, inertia, n_iter, tol_abs = lit.lloyd(Xs, C0, tol=tol, history=history)
    assert all(h["close"] == 0 for h in history), "%s: the literal meets close rows" % name
    if tol > 0:
        for h in history:
            if h["shift"] is not None:
                assert abs(h["shift"] - tol_abs) > 1e-6 * tol_abs, "%s: a shift at tol_abs" % name
    if name != "two_empty":
        assert np.array_equal(sk.labels_, labels), "%s: labels differ from scikit-learn" % name
        assert sk.n_iter_ == n_iter, "%s: n_iter_ %d, literal %d" % (name, sk.n_iter_, n_iter)
        bound = Xs.shape[0] * lit.EPS * np.abs(Xs).max()
        assert np.abs(sk.cluster_centers_ - C).max() <= bound
        assert abs(sk.inertia_ - inertia) <= Xs.shape[0] * lit.EPS * inertia
    assert k <= 256
    return {prefix + "labels": sk.labels_.astype(np.uint8), prefix + "centres": sk.cluster_centers_,
            prefix + "inertia": np.float64(sk.inertia_), prefix + "n_iter": np.int64(sk.n_iter_),
            prefix + "tol_abs": np.float64(tol_abs)}


def main():
    for name in cases.SCALER_ONLY_CASES:
        np.savez_compressed(os.path.join(HERE, "clustering_%s.npz" % name),
                            **scaler_golden(cases.scaler_case(name)))
    for name in cases.GOLDEN_CASES:
        case = cases.kmeans_case(name)
        out = scaler_golden(case["X"])
        out.update(kmeans_golden(name, case, 0.0, "t0_"))
        out.update(kmeans_golden(name, case, 1e-4, "td_"))
        if name == "one_empty":
            _, mind, _ = lit.assign(case["Xs"], case["C0"])
            top = np.sort(mind)[-2:]
            assert top[1] > top[0], "the farthest row is not unique"
            assert np.bincount(lit.assign(case["Xs"], case["C0"])[0], minlength=case["k"]).min() == 0
        path = os.path.join(HERE, "clustering_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%-22s n_iter tol0 %3d default %3d  %6d bytes" %
              (name, out["t0_n_iter"], out["td_n_iter"], os.path.getsize(path)))
    # the two-empty case has no scikit-learn golden; its conditions still hold
    case = cases.kmeans_case("two_empty")
    kmeans_golden("two_empty", case, 0.0, "t0_")
    kmeans_golden("two_empty", case, 1e-4, "td_")
    counts = np.bincount(lit.assign(case["Xs"], case["C0"])[0], minlength=case["k"])
    assert (counts == 0).sum() == 2, "two clusters must be empty at the first iteration"


if __name__ == "__main__":
    main()
