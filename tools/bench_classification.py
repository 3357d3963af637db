#!/usr/bin/env python3
"""The supervised classification tool at the reference's
batch size on one MI355X: 10^6 objects x 20 and x 100 features.

Per shape a 24-tree unlimited-depth forest and an rbf SVC are trained by
scikit-learn on about 1,000 labelled rows of three overlapping classes (the
models are what is measured, not the training).  With X resident on the device:
  * a forest predict batch on the LDS route and on the forced memory route:
    HIP-event time of the kernel and wall time of ``tmh_forest_predict_device``
    (which holds the finite-value census and the float32-range count as well);
  * an SVC predict batch, scaled on load, with the model's own tile and with
    the tile capped at 8 support vectors (the streamed route): event and wall
    time of ``tmh_svc_predict_device``;
  * beside each the box's flat read of X's bytes (``tmh_box_probe_device``).
scikit-learn's ``predict`` on the CPUs granted to the process is timed on the
first ``--cpu-rows`` rows (libsvm is single-threaded and takes tens of seconds
for 10^6 rows) and compared with the device's labels on those rows.

    python tools/bench_classification.py [--out profiles/r18/bench_classification.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_clustering import events, median_wall  # noqa: E402
from bench_jterator import box_rates  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.tools.base import DeviceTable, RobustScaler  # noqa: E402
from tmlibrary_amd.tools.supervised import ForestModel, SVCModel  # noqa: E402

SHAPES = ((10 ** 6, 20), (10 ** 6, 100))
CLASSES = 3
N_TRAIN = 1000


def features(n, d, seed):
    """three overlapping groups on feature scales from 0.5 to 50 -> (X, group)"""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-1.0, 1.0, size=(CLASSES, d))
    y = rs.randint(CLASSES, size=n)
    X = rs.normal(size=(n, d))
    X += centres[y]
    X *= rs.uniform(0.5, 50.0, size=d)
    X += rs.uniform(-100.0, 100.0, size=d)
    return X, y


def train(X, y):
    """-> (forest, svc, sklearn's scaler) fitted on the labelled rows"""
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.preprocessing import RobustScaler as SkScaler
    from sklearn.svm import SVC
    rf = RandomForestClassifier(n_estimators=24, max_depth=None, n_jobs=1, random_state=0).fit(X, y)
    sc = SkScaler(quantile_range=(1.0, 99.0)).fit(X)
    svc = SVC(kernel="rbf", C=8.0, gamma="scale", cache_size=500).fit(sc.transform(X), y)
    return rf, svc, sc


def timed(L, fn, scope, a, flat_ms):
    wall = median_wall(fn, a.warmup, a.reps)
    ev, _ = events(L, fn, (scope,), a.reps)
    return {"event_ms": round(ev, 4), "wall_ms": round(wall, 4), "x_flat_read": round(ev / flat_ms, 1)}


def bench_shape(L, n, d, a, read_gbs):
    import sklearn
    print("making %d x %d" % (n, d), file=sys.stderr, flush=True)
    X, y = features(n, d, 2000 + d)
    flat_ms = X.nbytes / (read_gbs * 1e6)
    rf, svc, sk_scaler = train(X[:N_TRAIN], y[:N_TRAIN].astype(np.float64))
    forest, svm = ForestModel.from_sklearn(rf), SVCModel.from_sklearn(svc)
    scaler = RobustScaler()
    scaler.center_, scaler.scale_, scaler.n_features_in_ = sk_scaler.center_, sk_scaler.scale_, d
    out = {"n": n, "d": d, "classes": CLASSES, "n_train": N_TRAIN, "x_bytes": X.nbytes,
           "flat_read_ms": round(flat_ms, 4)}
    pairs = svm.rho.size
    with DeviceTable(X, scaler) as t:
        dev_labels = t.alloc(4 * n)
        dev_values = t.alloc(8 * n * max(CLASSES, pairs))

        def forest_predict(proba=False):
            hip.check(L.tmh_forest_predict_device(forest.handle(), t.x, n, dev_labels,
                                                  dev_values if proba else None, None))

        def svc_predict():
            hip.check(L.tmh_svc_predict_device(svm.handle(), t.x, n, t.center, t.scale, dev_labels,
                                               None, None))

        route, nodes = forest.route()
        fo = {"trees": int(forest.tree_root.size), "packed_nodes": nodes,
              "packed_bytes": 16 * nodes, "route": route}
        fo["lds_route" if route == "lds" else "memory_route"] = timed(
            L, forest_predict, "forest_predict_" + ("lds" if route == "lds" else "mem"), a, flat_ms)
        fo["with_proba"] = timed(L, lambda: forest_predict(True),
                                 "forest_predict_" + ("lds" if route == "lds" else "mem"), a, flat_ms)
        forest_predict()
        f_labels = dev_labels.get(n, np.int32)
        hip.check(L.tmh_synchronize(None))
        if route == "lds":
            forest.memory_route = True
            assert forest.route()[0] == "memory"
            fo["memory_route"] = timed(L, forest_predict, "forest_predict_mem", a, flat_ms)
        out["forest"] = fo

        tile, tiles = svm.tile()
        so = {"support_vectors": int(svm.sv.shape[0]), "gamma": svm.gamma, "tile": tile,
              "tiles": tiles, "one_route": timed(L, svc_predict, "svc_predict", a, flat_ms)}
        svc_predict()
        s_labels = dev_labels.get(n, np.int32)
        hip.check(L.tmh_synchronize(None))
        svm.tile_cap = 8
        so["streamed_tile"], so["streamed_tiles"] = svm.tile()
        so["streamed_route"] = timed(L, svc_predict, "svc_predict", a, flat_ms)
        # n m d subtract-FMA pairs and n m exponentials, at 2 flops a pair
        so["f64_gflops"] = round(2.0 * n * svm.sv.shape[0] * d / (so["one_route"]["event_ms"] * 1e6), 1)
        out["svc"] = so
    forest.close()
    svm.close()
    if a.no_cpu:
        return out
    print("device done, CPU side", file=sys.stderr, flush=True)
    rows = min(n, a.cpu_rows)
    t0 = time.perf_counter()
    cpu_f = rf.predict(X[:rows])
    t1 = time.perf_counter()
    cpu_s = svc.predict(sk_scaler.transform(X[:rows]))
    t2 = time.perf_counter()
    scale_up = n / rows
    out["cpu"] = {"what": "scikit-learn %s, %s threads, on the first %d rows"
                          % (sklearn.__version__, os.environ.get("OMP_NUM_THREADS", "all"), rows),
                  "rows": rows, "forest_predict_ms": round((t1 - t0) * 1e3, 3),
                  "svc_predict_ms": round((t2 - t1) * 1e3, 3),
                  "forest_predict_ms_per_batch": round((t1 - t0) * 1e3 * scale_up, 1),
                  "svc_predict_ms_per_batch": round((t2 - t1) * 1e3 * scale_up, 1),
                  "note": "the per-batch figures are the measured ones times n / rows"}
    out["forest_labels_equal_cpu"] = float(np.mean(rf.classes_[f_labels[:rows]] == cpu_f))
    out["svc_labels_equal_cpu"] = float(np.mean(svc.classes_[s_labels[:rows]] == cpu_s))
    key = "lds_route" if out["forest"]["route"] == "lds" else "memory_route"
    out["x_cpu"] = {"forest": round(out["cpu"]["forest_predict_ms_per_batch"]
                                    / out["forest"][key]["wall_ms"], 1),
                    "svc": round(out["cpu"]["svc_predict_ms_per_batch"]
                                 / out["svc"]["one_route"]["wall_ms"], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="the device side alone (under a profiler)")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of 10^6 (a rehearsal)")
    ap.add_argument("--features", type=int, default=0,
                    help="only the shape with this many features (a counter run)")
    ap.add_argument("--cpu-rows", type=int, default=10 ** 5,
                    help="rows scikit-learn's predict is timed on")
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "bench_classification.json"))
    a = ap.parse_args()
    L = hip.lib()
    _, read_gbs = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_classification", "flat_read_gb_per_s": round(read_gbs, 1), "shapes": []}
    for n, d in SHAPES:
        if a.features and d != a.features:
            continue
        doc["shapes"].append(bench_shape(L, a.rows or n, d, a, read_gbs))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
