"""Supervised classifiers: training in scikit-learn, prediction on the GPU.

Mirrors tmlib/tools/base.py:502-584 (``Classifier.train_supervised``) and the
``model.predict`` of base.py:621-645.  Training sets are a few hundred rows, so
the grid-searched fit stays in scikit-learn on the host (imported only when a
model is trained or exported); the fitted estimator is exported into a flat
model -- plain arrays -- and every prediction runs from that model through the
C-ABI (``tmh_forest_predict`` / ``tmh_svc_predict``).  There is no CPU path for
prediction, and nothing on it imports scikit-learn.

``ForestModel`` gives ``RandomForestClassifier.predict`` / ``predict_proba`` of
scikit-learn 1.7.2 exactly; ``SVCModel`` gives libsvm's one-vs-one votes with
decision values that agree with libsvm's within rounding (include/tmhip.h
states both rules).
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.tools.base import MAX_FEATURES, MAX_ROWS, RobustScaler, as_table
from tmlibrary_amd.workflow.align.api import NotSupportedError

logger = logging.getLogger(__name__)

#: include/tmhip.h TMH_FOREST_MAX_* / TMH_SVC_MAX_*
MAX_FOREST_CLASSES = 64
MAX_FOREST_TREES = 256
MAX_FOREST_NODES = 2 ** 24
MAX_SVC_CLASSES = 16
MAX_SVC_VECTORS = 65536
SVC_KERNELS = {"rbf": hip.TMH_SVC_RBF, "linear": hip.TMH_SVC_LINEAR}


def _sklearn(what):
    try:
        import sklearn  # noqa: F401
    except ImportError:
        raise NotSupportedError("%s needs scikit-learn, which is not installed." % what)
    return sklearn


def _check_table_limits(n, d):
    if d > MAX_FEATURES:
        raise NotSupportedError("%d features: at most %d are supported." % (d, MAX_FEATURES))
    if n > MAX_ROWS:
        raise NotSupportedError("%d rows: at most 2**31 - 1 are supported." % n)


class _FlatModel(object):
    """What the two models share: the lazily created handle and the table checks."""

    _destroy = None

    def __init__(self):
        self._handle = None

    def _create(self, L):
        raise NotImplementedError

    def handle(self):
        if self._handle is None:
            self._handle = self._create(hip.lib())
        return self._handle

    def close(self):
        if self._handle is not None:
            getattr(hip.lib(), self._destroy)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _table(self, X):
        X = as_table(X)
        n, d = X.shape
        if d != self.n_features_in_:
            raise ValueError("X has %d features, but %s is expecting %d features as input."
                             % (d, type(self).__name__, self.n_features_in_))
        _check_table_limits(n, d)
        return X


class ForestModel(_FlatModel):
    """A fitted ``RandomForestClassifier`` as flat arrays.

    ``feature`` [nodes] (-1: a leaf), ``threshold`` [nodes], ``left`` / ``right``
    [nodes], ``tree_root`` [n_trees], ``leaf_row`` [nodes], ``leaf_value``
    [n_leaves][n_classes], ``n_features`` and ``classes`` -- the npz form of
    ``to_arrays`` / ``from_arrays``."""

    _destroy = "tmh_forest_destroy"

    def __init__(self, feature, threshold, left, right, tree_root, leaf_row, leaf_value,
                 n_features, classes):
        super(ForestModel, self).__init__()
        self.n_features_in_ = int(n_features)
        self.classes_ = np.asarray(classes)
        # the limits first, on the sizes alone: nothing over them is converted
        self._check_limits(np.asarray(tree_root).size, np.asarray(feature).size)
        self.feature = np.ascontiguousarray(feature, dtype=np.int32)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        self.left = np.ascontiguousarray(left, dtype=np.int32)
        self.right = np.ascontiguousarray(right, dtype=np.int32)
        self.tree_root = np.ascontiguousarray(tree_root, dtype=np.int32)
        self.leaf_row = np.ascontiguousarray(leaf_row, dtype=np.int32)
        self.leaf_value = np.ascontiguousarray(leaf_value, dtype=np.float64)
        nodes = self.feature.size
        if not (self.threshold.shape == self.left.shape == self.right.shape
                == self.leaf_row.shape == (nodes,)) or self.tree_root.ndim != 1:
            raise ValueError("the node arrays must have one entry per node")
        if self.leaf_value.ndim != 2 or self.leaf_value.shape[1] != self.classes_.size:
            raise ValueError("leaf_value must have shape (n_leaves, n_classes)")
        self.memory_route = False

    def _check_limits(self, trees, nodes):
        d, c = self.n_features_in_, self.classes_.size
        if not 1 <= d <= MAX_FEATURES:
            raise NotSupportedError("%d features: at most %d are supported." % (d, MAX_FEATURES))
        if not 2 <= c <= MAX_FOREST_CLASSES:
            raise NotSupportedError("%d classes: a forest of 2 to %d classes is supported."
                                    % (c, MAX_FOREST_CLASSES))
        if not 1 <= trees <= MAX_FOREST_TREES:
            raise NotSupportedError("%d trees: 1 to %d trees are supported."
                                    % (trees, MAX_FOREST_TREES))
        if not 1 <= nodes < MAX_FOREST_NODES:
            raise NotSupportedError("%d nodes: fewer than 2**24 nodes are supported." % nodes)

    @classmethod
    def from_sklearn(cls, estimator):
        """The flat model of a fitted single-output ``RandomForestClassifier``."""
        _sklearn("Exporting a forest")
        if getattr(estimator, "n_outputs_", 1) != 1:
            raise NotSupportedError("Forests with more than one output are not supported.")
        n_classes = len(estimator.classes_)
        parts = {k: [] for k in ("feature", "threshold", "left", "right", "leaf_row", "value")}
        roots, at, leaves = [], 0, 0
        for est in estimator.estimators_:
            t = est.tree_
            is_leaf = t.children_left < 0
            roots.append(at)
            parts["feature"].append(np.where(is_leaf, -1, t.feature))
            parts["threshold"].append(np.where(is_leaf, 0.0, t.threshold))
            parts["left"].append(np.where(is_leaf, 0, t.children_left + at))
            parts["right"].append(np.where(is_leaf, 0, t.children_right + at))
            row = np.zeros(t.node_count, dtype=np.int64)
            row[is_leaf] = leaves + np.arange(int(is_leaf.sum()))
            parts["leaf_row"].append(row)
            parts["value"].append(t.value[is_leaf, 0, :n_classes])
            at += t.node_count
            leaves += int(is_leaf.sum())
        cat = {k: np.concatenate(v) for k, v in parts.items()}
        return cls(cat["feature"], cat["threshold"], cat["left"], cat["right"], roots,
                   cat["leaf_row"], cat["value"], estimator.n_features_in_, estimator.classes_)

    def to_arrays(self):
        return {"feature": self.feature, "threshold": self.threshold, "left": self.left,
                "right": self.right, "tree_root": self.tree_root, "leaf_row": self.leaf_row,
                "leaf_value": self.leaf_value, "n_features": np.int64(self.n_features_in_),
                "classes": self.classes_}

    @classmethod
    def from_arrays(cls, **a):
        return cls(a["feature"], a["threshold"], a["left"], a["right"], a["tree_root"],
                   a["leaf_row"], a["leaf_value"], int(a["n_features"]), a["classes"])

    def _create(self, L):
        h = C.c_void_p()
        hip.check(L.tmh_forest_create(
            hip.ptr(self.feature), hip.ptr(self.threshold), hip.ptr(self.left), hip.ptr(self.right),
            hip.ptr(self.leaf_row), self.feature.size, hip.ptr(self.tree_root), self.tree_root.size,
            hip.ptr(self.leaf_value), self.leaf_value.shape[0], self.classes_.size,
            self.n_features_in_, C.byref(h)))
        return h

    def route(self):
        """-> ("lds" | "memory", packed nodes): the route a predict takes now."""
        L = hip.lib()
        h = self.handle()
        hip.check(L.tmh_forest_set_option(h, hip.TMH_OPT_FOREST_MEMORY_ROUTE,
                                          int(self.memory_route)))
        route, nodes = C.c_int(0), C.c_int64(0)
        hip.check(L.tmh_forest_route(h, C.byref(route), C.byref(nodes)))
        return ("lds" if route.value == hip.TMH_FOREST_ROUTE_LDS else "memory"), nodes.value

    @staticmethod
    def _check_input(X):
        if not np.isfinite(X).all():
            raise ValueError("Input X contains NaN or infinity.")
        with np.errstate(over="ignore"):
            if not np.isfinite(X.astype(np.float32)).all():
                raise ValueError("Input X contains a value too large for dtype('float32').")

    def _run(self, X, scaler, want_proba):
        X = self._table(X)
        if scaler is not None:      # the reference trains forests without one
            X = scaler.transform(X)
        self._check_input(X)
        n = X.shape[0]
        L = hip.lib()
        h = self.handle()
        hip.check(L.tmh_forest_set_option(h, hip.TMH_OPT_FOREST_MEMORY_ROUTE,
                                          int(self.memory_route)))
        labels = np.empty(n, dtype=np.int32)
        proba = np.empty((n, self.classes_.size), dtype=np.float64) if want_proba else None
        hip.check(L.tmh_forest_predict(h, hip.ptr(X), n, hip.ptr(labels), hip.ptr_or_null(proba)))
        return labels, proba

    def predict(self, X, scaler=None):
        return self.classes_[self._run(X, scaler, False)[0]]

    def predict_proba(self, X, scaler=None):
        return self._run(X, scaler, True)[1]


class SVCModel(_FlatModel):
    """A fitted ``SVC`` as flat arrays, in libsvm's own sign convention.

    ``kernel`` ("rbf" or "linear"), ``gamma``, ``sv`` [m][d] grouped by class,
    ``n_sv`` [k], ``coef`` [k - 1][m] (``_dual_coef_``), ``rho`` [k (k - 1) / 2]
    (``-_intercept_``) and ``classes``."""

    _destroy = "tmh_svc_destroy"

    def __init__(self, kernel, gamma, sv, n_sv, coef, rho, classes):
        super(SVCModel, self).__init__()
        kernel = str(kernel)
        if kernel not in SVC_KERNELS:
            raise NotSupportedError('SVC kernel "%s": "rbf" and "linear" are supported.' % kernel)
        self.kernel = kernel
        self.gamma = float(gamma)
        self.sv = np.ascontiguousarray(sv, dtype=np.float64)
        self.n_sv = np.ascontiguousarray(n_sv, dtype=np.int32)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.rho = np.ascontiguousarray(rho, dtype=np.float64)
        self.classes_ = np.asarray(classes)
        if self.sv.ndim != 2:
            raise ValueError("sv must have shape (n_vectors, n_features)")
        m, d = self.sv.shape
        k = self.classes_.size
        self.n_features_in_ = d
        if not 1 <= d <= MAX_FEATURES:
            raise NotSupportedError("%d features: at most %d are supported." % (d, MAX_FEATURES))
        if not 2 <= k <= MAX_SVC_CLASSES:
            raise NotSupportedError("%d classes: an SVC of 2 to %d classes is supported."
                                    % (k, MAX_SVC_CLASSES))
        if not 1 <= m <= MAX_SVC_VECTORS:
            raise NotSupportedError("%d support vectors: 1 to %d are supported."
                                    % (m, MAX_SVC_VECTORS))
        if self.n_sv.shape != (k,) or self.coef.shape != (k - 1, m) or \
                self.rho.shape != (k * (k - 1) // 2,):
            raise ValueError("n_sv, coef and rho must have shapes (k,), (k - 1, m) and "
                             "(k (k - 1) / 2,)")
        self.tile_cap = 0

    @classmethod
    def from_sklearn(cls, estimator):
        """The flat model of a fitted dense ``SVC`` (C-SVC, rbf or linear)."""
        _sklearn("Exporting an SVC")
        if getattr(estimator, "_sparse", False):
            raise NotSupportedError("SVCs fitted on sparse data are not supported.")
        return cls(estimator.kernel, estimator._gamma, estimator.support_vectors_,
                   estimator.n_support_, estimator._dual_coef_, -estimator._intercept_,
                   estimator.classes_)

    def to_arrays(self):
        return {"kernel": np.str_(self.kernel), "gamma": np.float64(self.gamma), "sv": self.sv,
                "n_sv": self.n_sv, "coef": self.coef, "rho": self.rho, "classes": self.classes_}

    @classmethod
    def from_arrays(cls, **a):
        return cls(str(a["kernel"]), float(a["gamma"]), a["sv"], a["n_sv"], a["coef"], a["rho"],
                   a["classes"])

    def _create(self, L):
        h = C.c_void_p()
        m, d = self.sv.shape
        hip.check(L.tmh_svc_create(SVC_KERNELS[self.kernel], self.gamma, hip.ptr(self.sv), m, d,
                                   hip.ptr(self.n_sv), self.classes_.size, hip.ptr(self.coef),
                                   hip.ptr(self.rho), C.byref(h)))
        return h

    def tile(self):
        """-> (support vectors per LDS tile, tiles) under the current ``tile_cap``."""
        L = hip.lib()
        h = self.handle()
        hip.check(L.tmh_svc_set_option(h, hip.TMH_OPT_SVC_TILE, int(self.tile_cap)))
        tile, tiles = C.c_int(0), C.c_int(0)
        hip.check(L.tmh_svc_tile(h, C.byref(tile), C.byref(tiles)))
        return tile.value, tiles.value

    def _run(self, X, scaler, want_dec):
        X = self._table(X)
        if not np.isfinite(X).all():
            raise ValueError("Input X contains NaN or infinity.")
        n, d = X.shape
        if scaler is not None:
            scaler._check_fitted(d)
        L = hip.lib()
        h = self.handle()
        hip.check(L.tmh_svc_set_option(h, hip.TMH_OPT_SVC_TILE, int(self.tile_cap)))
        labels = np.empty(n, dtype=np.int32)
        pairs = self.rho.size
        dec = np.empty((n, pairs), dtype=np.float64) if want_dec else None
        hip.check(L.tmh_svc_predict(
            h, hip.ptr(X), n, None if scaler is None else hip.ptr(scaler.center_),
            None if scaler is None else hip.ptr(scaler.scale_), hip.ptr(labels),
            hip.ptr_or_null(dec)))
        return labels, dec

    def predict(self, X, scaler=None):
        return self.classes_[self._run(X, scaler, False)[0]]

    def decision_function(self, X, scaler=None):
        """The pairs' decision values [n][k (k - 1) / 2] in libsvm's sign and order
        (for two classes the negative of scikit-learn's ``decision_function``)."""
        return self._run(X, scaler, True)[1]


def search_spaces():
    """The reference's estimators' search spaces (base.py:524-551)."""
    return {
        "randomforest": {"n_estimators": [3, 6, 12, 24], "max_depth": [3, 6, 12, None],
                         "min_samples_split": [2, 4, 8], "class_weight": ["balanced", None]},
        "svm": {"kernel": ["linear", "rbf"], "C": np.logspace(-5, 15, 10, base=2),
                "gamma": np.logspace(-15, -3, 10, base=2)},
    }


def train_supervised(feature_data, labels, method, n_fold_cv, random_state=None):
    """-> (model, scaler): base.py:524-584 for ``randomforest`` and ``svm``.

    The same estimators, search spaces, ``KFold(n_fold_cv)`` and ``GridSearchCV``
    as the reference, fitted by scikit-learn on the host; ``best_estimator_`` is
    exported as a ``ForestModel`` / ``SVCModel``.  The SVM's scaler is
    scikit-learn's ``RobustScaler(quantile_range=(1, 99))``, handed back as this
    project's ``RobustScaler`` carrying its ``center_`` / ``scale_`` (``None`` for
    the forest).  ``labels`` maps mapobject id to label; ``feature_data`` needs
    an ``.index`` of mapobject ids.  ``random_state`` seeds the forest (the
    reference's is unseeded and so not repeatable)."""
    if method == "logisticregression":
        raise NotSupportedError("Logistic regression is not built: the reference's tool does not "
                                "offer it.")
    if method not in ("randomforest", "svm"):
        raise ValueError('Unknown method "%s".' % method)
    _sklearn("Supervised training")
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import GridSearchCV, KFold
    from sklearn.preprocessing import RobustScaler as SkRobustScaler
    from sklearn.svm import SVC

    index = getattr(feature_data, "index", None)
    if index is None:
        raise ValueError("feature_data needs an index of mapobject ids")
    logger.info('train "%s" classifier', method)
    y = np.array([labels[int(i)] for i in np.asarray(index)])
    X = as_table(feature_data)
    if not np.isfinite(X).all():
        raise ValueError("Input X contains NaN or infinity.")
    scaler = None
    if method == "svm":
        sk_scaler = SkRobustScaler(quantile_range=(1.0, 99.0)).fit(X)
        scaler = RobustScaler(quantile_range=(1.0, 99.0))
        scaler.center_ = np.ascontiguousarray(sk_scaler.center_, dtype=np.float64)
        scaler.scale_ = np.ascontiguousarray(sk_scaler.scale_, dtype=np.float64)
        scaler.n_features_in_ = X.shape[1]
        X = (X - scaler.center_) / scaler.scale_    # what tmh_robust_scale writes
        clf = SVC(cache_size=500, decision_function_shape="ovr")
    else:
        clf = RandomForestClassifier(n_jobs=1, random_state=random_state)
    search = GridSearchCV(clf, search_spaces()[method], cv=KFold(n_splits=n_fold_cv))
    search.fit(X, y)
    best = search.best_estimator_
    model = SVCModel.from_sklearn(best) if method == "svm" else ForestModel.from_sklearn(best)
    return (model, scaler)
