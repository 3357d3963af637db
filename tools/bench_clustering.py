#!/usr/bin/env python3
"""The clustering tool at the reference's batch size on
one MI355X: 10^6 objects x 20 features at k = 8 and x 100 features at k = 20.

Per shape, with X resident on the device:
  * the scaler fit (census + six order statistics per column): HIP-event time
    of ``column_census`` + ``column_select`` and the wall time of the two calls;
  * one Lloyd iteration: HIP-event time of ``kmeans_assign`` + ``kmeans_update``
    per iteration of a fit;
  * a whole fit from k-means++ centres (``tmh_kmeans_seed_device`` then
    ``tmh_kmeans_fit_device``, scaled on load, at most ``--max-iter``
    iterations): wall time of each call, and the seeding's event time;
  * a predict batch: event and wall time of ``tmh_kmeans_predict_device``;
  * beside each the box's flat read of X's bytes (``tmh_box_probe_device``).
The same work on the CPUs granted to the process: scikit-learn where it
imports (RobustScaler.fit, KMeans(init=the same centres, n_init=1).fit,
predict), else the numpy literal of tests/clustering_literal.py.  The device's
labels are compared with the CPU's.

    python tools/bench_clustering.py [--out profiles/r17/bench_clustering.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_jterator import box_rates  # noqa: E402
from bench_pyramid import kernel_ms  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.tools.base import DeviceTable, KMeans, RobustScaler  # noqa: E402

SHAPES = ((10 ** 6, 20, 8), (10 ** 6, 100, 20))


def features(n, d, k, seed):
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-1.0, 1.0, size=(k, d))   # overlapping groups: Lloyd has work to do
    X = rs.normal(size=(n, d))
    X += centres[rs.randint(k, size=n)]
    X *= rs.uniform(0.5, 50.0, size=d)
    X += rs.uniform(-100.0, 100.0, size=d)
    return X


def median_wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append(time.perf_counter() - t0)
    return float(np.median(walls)) * 1e3


def events(L, fn, names, reps):
    """summed HIP-event ms per call of the named scopes, and their launches per call"""
    hip.check(L.tmh_profile_enable(1))
    hip.check(L.tmh_profile_reset())
    for _ in range(reps):
        fn()
    got = [kernel_ms(L, name) for name in names]
    hip.check(L.tmh_profile_enable(0))
    return sum(ms for ms, _ in got) / reps, [cnt // reps for _, cnt in got]


def cpu_side(X, C0_scaled, max_iter, tol):
    try:
        from sklearn.cluster import KMeans as SkKMeans
        from sklearn.preprocessing import RobustScaler as SkScaler
    except ImportError:
        import clustering_literal as lit
        t0 = time.perf_counter()
        center, scale = lit.robust_fit(X)
        t1 = time.perf_counter()
        Xs = lit.robust_transform(X, center, scale)
        t2 = time.perf_counter()
        labels, C_, inertia, n_iter, _ = lit.lloyd(Xs, C0_scaled, max_iter=max_iter, tol=tol)
        t3 = time.perf_counter()
        lit.assign(Xs, C_)
        t4 = time.perf_counter()
        return {"what": "numpy literal", "scaler_fit_ms": (t1 - t0) * 1e3,
                "fit_ms": (t3 - t2) * 1e3, "n_iter": n_iter, "predict_ms": (t4 - t3) * 1e3,
                "inertia": inertia}, labels
    import sklearn
    t0 = time.perf_counter()
    sc = SkScaler(quantile_range=(1.0, 99.0)).fit(X)
    t1 = time.perf_counter()
    Xs = sc.transform(X)
    t2 = time.perf_counter()
    km = SkKMeans(n_clusters=C0_scaled.shape[0], init=C0_scaled, n_init=1, algorithm="lloyd",
                  max_iter=max_iter, tol=tol).fit(Xs)
    t3 = time.perf_counter()
    km.predict(Xs)
    t4 = time.perf_counter()
    return {"what": "scikit-learn %s, %s threads" % (sklearn.__version__,
                                                     os.environ.get("OMP_NUM_THREADS", "all")),
            "scaler_fit_ms": (t1 - t0) * 1e3, "transform_ms": (t2 - t1) * 1e3,
            "fit_ms": (t3 - t2) * 1e3, "n_iter": int(km.n_iter_),
            "ms_per_iteration": (t3 - t2) * 1e3 / km.n_iter_, "predict_ms": (t4 - t3) * 1e3,
            "inertia": float(km.inertia_)}, km.labels_


def bench_shape(L, n, d, k, a, read_gbs):
    print("making %d x %d" % (n, d), file=sys.stderr, flush=True)
    X = features(n, d, k, 1000 + d)
    flat_ms = X.nbytes / (read_gbs * 1e6)
    scaler = RobustScaler()
    count, n_inf = np.zeros(d, np.int64), np.zeros(d, np.int64)
    ranks = np.zeros((d, 6), np.int64)
    ranks[:], _ = RobustScaler.column_ranks(n, (1.0, 99.0))
    values = np.zeros((d, 6))
    out = {"n": n, "d": d, "k": k, "x_bytes": X.nbytes, "flat_read_ms": round(flat_ms, 4)}
    with DeviceTable(X) as t:
        def scaler_fit():
            hip.check(L.tmh_column_census_device(t.x, n, d, None, None, hip.ptr(count),
                                                 hip.ptr(n_inf), None, None, None))
            hip.check(L.tmh_column_select_device(t.x, n, d, hip.ptr(count), hip.ptr(ranks), 6,
                                                 hip.ptr(values), None))
        wall = median_wall(scaler_fit, a.warmup, a.reps)
        ev, _ = events(L, scaler_fit, ("column_census", "column_select"), a.reps)
        out["scaler_fit"] = {"event_ms": round(ev, 4), "wall_ms": round(wall, 4),
                             "x_flat_read": round(ev / flat_ms, 1)}
    scaler.fit(X)
    with DeviceTable(X, scaler) as t:
        rs = np.random.RandomState(7)
        trials = KMeans.n_local_trials(k)
        first = rs.randint(n)
        draws = np.array([rs.uniform(size=trials) for _ in range(k - 1)])
        seeded = {}

        def seed():
            seeded["c"] = KMeans.seed(t, k, first, draws)[1]
        seed_wall = median_wall(seed, a.warmup, a.reps)
        seed_ev, _ = events(L, seed, ("kmeans_seed",), a.reps)
        C0 = seeded["c"]
        dev_labels = t.alloc(4 * n)
        centres = np.zeros((k, d))
        inertia, tol_abs, n_iter = C.c_double(), C.c_double(), C.c_int()

        def fit(max_iter=a.max_iter, tol=1e-4):
            hip.check(L.tmh_kmeans_fit_device(t.x, n, d, k, t.center, t.scale, hip.ptr(C0),
                                              max_iter, tol, hip.ptr(centres), dev_labels,
                                              C.byref(inertia), C.byref(n_iter), C.byref(tol_abs),
                                              None))
        fit_wall = median_wall(fit, a.warmup, a.reps)
        iters = n_iter.value
        as_ev, launches = events(L, lambda: fit(5, 0.0), ("kmeans_assign",), a.reps)
        up_ev, _ = events(L, lambda: fit(5, 0.0), ("kmeans_update",), a.reps)
        short = n_iter.value
        # the closing assign (no sums) is counted in when the labels still moved
        per_iter = (as_ev + up_ev) / short
        fit()
        labels = dev_labels.get(n, np.int32)
        hip.check(L.tmh_synchronize(None))
        dev_inertia = inertia.value

        def predict():
            hip.check(L.tmh_kmeans_predict_device(t.x, n, d, k, t.center, t.scale,
                                                  hip.ptr(centres), dev_labels, None, None))
        pred_wall = median_wall(predict, a.warmup, a.reps)
        pred_ev, _ = events(L, predict, ("kmeans_assign",), a.reps)
        out["seed"] = {"event_ms": round(seed_ev, 4), "wall_ms": round(seed_wall, 4),
                       "trials": trials, "x_flat_read": round(seed_ev / flat_ms, 1)}
        out["lloyd_iteration"] = {"event_ms": round(per_iter, 4),
                                  "assign_event_ms": round(as_ev / short, 4),
                                  "update_event_ms": round(up_ev / short, 4),
                                  "assign_launches": launches[0], "iterations": short,
                                  "x_flat_read": round(per_iter / flat_ms, 1)}
        out["fit"] = {"wall_ms": round(fit_wall, 3), "n_iter": iters, "max_iter": a.max_iter,
                      "tol": 1e-4, "inertia": dev_inertia,
                      "wall_ms_per_iteration": round(fit_wall / iters, 4)}
        out["predict"] = {"event_ms": round(pred_ev, 4), "wall_ms": round(pred_wall, 4),
                          "x_flat_read": round(pred_ev / flat_ms, 1),
                          "note": "the wall time holds the finite-value census as well"}
    if a.no_cpu:
        return out
    print("device done, CPU side", file=sys.stderr, flush=True)
    cpu, cpu_labels = cpu_side(X, C0, a.max_iter, 1e-4)
    out["cpu"] = {key: (round(v, 3) if isinstance(v, float) else v) for key, v in cpu.items()}
    out["labels_equal_cpu"] = float(np.mean(labels == cpu_labels))
    out["n_iter_equal_cpu"] = bool(iters == cpu["n_iter"])
    out["inertia_rel_diff"] = abs(dev_inertia - cpu["inertia"]) / cpu["inertia"]
    out["x_cpu"] = {"scaler_fit": round(cpu["scaler_fit_ms"] / out["scaler_fit"]["wall_ms"], 1),
                    "fit": round(cpu["fit_ms"] / out["fit"]["wall_ms"], 1),
                    "predict": round(cpu["predict_ms"] / out["predict"]["wall_ms"], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--no-cpu", action="store_true", help="the device side alone (under a profiler)")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of 10^6 (a rehearsal)")
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "bench_clustering.json"))
    a = ap.parse_args()
    L = hip.lib()
    _, read_gbs = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_clustering", "flat_read_gb_per_s": round(read_gbs, 1), "shapes": []}
    for n, d, k in SHAPES:
        doc["shapes"].append(bench_shape(L, a.rows or n, d, k, a, read_gbs))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
