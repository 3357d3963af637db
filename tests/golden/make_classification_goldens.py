"""Writes tests/golden/classification_<case>.npz: what scikit-learn computes for
the cases of tests/classification_cases.py.

    python tests/golden/make_classification_goldens.py

Per case the flat model arrays (``ForestModel.to_arrays`` / ``SVCModel.to_arrays``,
prefixed ``m_``), the table ``X`` and scikit-learn's answers: for a forest
``labels`` (indices into classes, uint8) and ``proba``; for an SVC ``labels``,
``dec`` (``decision_function`` of shape 'ovo' in libsvm's sign) and, where the
case has one, the scaler's ``center`` / ``scale``.

The generator asserts what the tests rely on and fails otherwise:
  * the forest literal (tests/classification_literal.py) equals ``predict_proba``
    bit for bit and ``predict`` without a mismatch;
  * the SVC literal has no label mismatch, meets NO close row, and its decision
    values lie within the close-row bound of scikit-learn's;
  * every exported model passes the literal's restatement of the validation;
  * every file stays under 130 KB.
"""
import os
import sys

import numpy as np
from sklearn.ensemble import RandomForestClassifier
from sklearn.preprocessing import RobustScaler
from sklearn.svm import SVC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import classification_cases as cases  # noqa: E402
import classification_literal as lit  # noqa: E402
from tmlibrary_amd.tools.supervised import ForestModel, SVCModel  # noqa: E402

LIMIT = 130 * 1024


def forest_golden(name, spec):
    Xt, y = cases.training_set(spec)
    rf = RandomForestClassifier(n_estimators=spec["trees"], max_depth=spec["depth"], n_jobs=1,
                                random_state=spec["seed"]).fit(Xt, y)
    at = spec.get("single_leaf_at")
    if at is not None:
        # a tree that never splits: its root is its only leaf
        stump = RandomForestClassifier(n_estimators=1, min_samples_split=10 ** 6, n_jobs=1,
                                       random_state=spec["seed"]).fit(Xt, y)
        rf.estimators_.insert(at, stump.estimators_[0])
        assert rf.estimators_[at].tree_.node_count == 1
    assert len(rf.estimators_) == spec["trees"] + (at is not None)
    model = ForestModel.from_sklearn(rf)
    arrays = model.to_arrays()
    assert lit.forest_validate(arrays) is None, "%s: the exported model is refused" % name
    X = cases.table(spec)
    proba = rf.predict_proba(X)
    labels, lit_proba = lit.forest_predict(arrays, X)
    assert lit_proba.tobytes() == proba.tobytes(), "%s: proba is not bit for bit" % name
    assert np.array_equal(rf.classes_[labels], rf.predict(X)), "%s: labels differ" % name
    out = {"m_" + k: v for k, v in arrays.items()}
    out.update(X=X, labels=labels.astype(np.uint8), proba=proba)
    return out, "%d trees, %d nodes" % (arrays["tree_root"].size, arrays["feature"].size)


def svc_golden(name, spec):
    Xt, y = cases.training_set(spec)
    X = cases.table(spec)
    out = {}
    if spec["scaler"]:
        sc = RobustScaler(quantile_range=(1.0, 99.0)).fit(Xt)
        out.update(center=sc.center_, scale=sc.scale_)
        Xt = lit.scale(Xt, sc.center_, sc.scale_)
        Xs = lit.scale(X, sc.center_, sc.scale_)
        assert np.array_equal(sc.transform(X), Xs)
    else:
        Xs = X
    svc = SVC(kernel=spec["kernel"], C=spec["C"], gamma=spec["gamma"], cache_size=500,
              decision_function_shape="ovo").fit(Xt, y)
    model = SVCModel.from_sklearn(svc)
    arrays = model.to_arrays()
    dec = svc.decision_function(Xs)
    if spec["classes"] == 2:
        dec = -dec.reshape(-1, 1)       # scikit-learn flips two classes; libsvm's sign
    want = svc.predict(Xs)
    labels, lit_dec, close = lit.svc_predict(arrays, Xs)
    assert close.sum() == 0, "%s: the literal meets %d close rows" % (name, close.sum())
    assert np.array_equal(svc.classes_[labels], want), "%s: labels differ" % name
    bound = lit.svc_dec_bound(arrays, Xs)
    assert (np.abs(lit_dec - dec) <= bound).all(), "%s: decision values past the bound" % name
    out.update({"m_" + k: v for k, v in arrays.items()})
    out.update(X=X, labels=labels.astype(np.uint8), dec=dec)
    return out, "m = %d, max |d dec| %.2g of bound %.2g" % (
        arrays["sv"].shape[0], np.abs(lit_dec - dec).max(), bound.min())


def main():
    for table, make in ((cases.FOREST_GOLDEN, forest_golden), (cases.SVC_GOLDEN, svc_golden)):
        for name, spec in table.items():
            out, note = make(name, spec)
            path = os.path.join(HERE, "classification_%s.npz" % name)
            np.savez_compressed(path, **out)
            size = os.path.getsize(path)
            assert size <= LIMIT, "%s: %d bytes" % (name, size)
            print("%-22s %7d bytes  %s" % (name, size, note))


if __name__ == "__main__":
    main()
