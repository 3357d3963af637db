"""Classification tools: the scaler, the model and the ``Classifier`` base.

Mirrors tmlib/tools/base.py:586-645 (``Classifier.train_unsupervised`` /
``predict``), where scikit-learn's ``RobustScaler(quantile_range=(1.0, 99.0))``
and ``KMeans(n_clusters=k)`` do the work.  Here both run on the GPU through the
C-ABI (``tmh_column_census`` / ``tmh_column_select`` / ``tmh_robust_scale`` /
``tmh_kmeans_seed`` / ``tmh_kmeans_fit`` / ``tmh_kmeans_predict``); there is no
CPU path.  numpy at the boundary: anything ``np.asarray`` accepts is taken, so
a DataFrame works; pandas is imported only to hand back a Series when the
input had an ``.index``.

Differences by design: the database is an in-memory ``FeatureStore``;
``KMeans`` runs ``n_init=1`` by default; the supervised models (random forest,
SVM with grid search) live in ``tools/supervised.py`` and the ``Classification``
tool overrides ``train_supervised``, which stays unbuilt on this base class.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.workflow.align.api import NotSupportedError
from tmlibrary_amd.workflow.corilla.quantiles import lerp, quantile_table

logger = logging.getLogger(__name__)

#: include/tmhip.h TMH_CLUSTER_MAX_*
MAX_FEATURES = 256
MAX_CLUSTERS = 64
MAX_CENTRE_VALUES = 8192
MAX_ROWS = 2 ** 31 - 1


def as_table(X):
    """X as a C-contiguous [n][d] f64 array"""
    a = np.ascontiguousarray(np.asarray(X), dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("Expected a 2D array of feature values, got %d dimension(s)." % a.ndim)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("Found an array with shape %r: at least one row and one feature are "
                         "required." % (a.shape,))
    return a


def check_limits(n, d, k=None):
    """What the kernels do not hold is refused by name, never computed wrongly."""
    if d > MAX_FEATURES:
        raise NotSupportedError("%d features: at most %d are supported." % (d, MAX_FEATURES))
    if n > MAX_ROWS:
        raise NotSupportedError("%d rows: at most 2**31 - 1 are supported." % n)
    if k is None:
        return
    if k > MAX_CLUSTERS:
        raise NotSupportedError("%d clusters: at most %d are supported." % (k, MAX_CLUSTERS))
    if k * d > MAX_CENTRE_VALUES:
        raise NotSupportedError("%d clusters of %d features: n_clusters * n_features may be at "
                                "most %d." % (k, d, MAX_CENTRE_VALUES))


class DeviceTable(object):
    """A feature table (and its optional scaler) in device memory for the
    length of a ``with`` block, so that one upload serves several calls."""

    def __init__(self, X, scaler=None):
        self.X = X
        self.n, self.d = X.shape
        self.scaler = scaler
        self._buffers = []
        self.x = self.center = self.scale = None

    def _upload(self, a):
        self._buffers.append(hip.DeviceBuffer.from_array(a))
        return self._buffers[-1]

    def alloc(self, nbytes):
        """A ``hip.DeviceBuffer`` that lives as long as the table."""
        self._buffers.append(hip.DeviceBuffer(nbytes))
        return self._buffers[-1]

    def __enter__(self):
        try:
            self.x = self._upload(self.X)
            if self.scaler is not None:
                self.center = self._upload(np.ascontiguousarray(self.scaler.center_, np.float64))
                self.scale = self._upload(np.ascontiguousarray(self.scaler.scale_, np.float64))
        except Exception:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        for buf in self._buffers:
            buf.free()
        self._buffers = []
        return False


class RobustScaler(object):
    """``sklearn.preprocessing.RobustScaler(quantile_range=...)``: ``center_`` is
    the median and ``scale_`` the quantile range of every feature, NaN ignored
    as ``np.nanmedian`` / ``np.nanpercentile`` do; a zero scale becomes 1."""

    def __init__(self, quantile_range=(1.0, 99.0)):
        q_min, q_max = quantile_range
        if not 0 <= q_min <= q_max <= 100:
            raise ValueError("Invalid quantile range: %s" % str(quantile_range))
        self.quantile_range = (float(q_min), float(q_max))

    @staticmethod
    def column_ranks(m, quantile_range):
        """The six 0-based ranks a column of m values needs -- the two middle
        values, (lo, hi) of each percentile -- and the two lerp weights."""
        lo, hi, gamma = quantile_table(m, np.array(quantile_range, dtype=np.float64))
        return [(m - 1) // 2, m // 2, lo[0], hi[0], lo[1], hi[1]], gamma

    @staticmethod
    def finish(values, gammas):
        """center_ and scale_ from the order statistics [d][6] and weights [d][2]"""
        values = np.asarray(values, dtype=np.float64)
        gammas = np.asarray(gammas, dtype=np.float64)
        # the median is the mean of the two middle values, not the 50 % lerp
        center = (values[:, 0] + values[:, 1]) / 2
        scale = lerp(values[:, 4], values[:, 5], gammas[:, 1]) - \
            lerp(values[:, 2], values[:, 3], gammas[:, 0])
        scale = np.where(scale == 0.0, 1.0, scale)   # sklearn's _handle_zeros_in_scale
        return center, scale

    def fit(self, X, y=None):
        X = as_table(X)
        n, d = X.shape
        check_limits(n, d)
        L = hip.lib()
        with DeviceTable(X) as t:
            count = np.zeros(d, dtype=np.int64)
            n_inf = np.zeros(d, dtype=np.int64)
            hip.check(L.tmh_column_census_device(t.x, n, d, None, None, hip.ptr(count),
                                                 hip.ptr(n_inf), None, None, None))
            if (count == 0).any():
                raise ValueError("Feature %d holds no value other than NaN."
                                 % int(np.flatnonzero(count == 0)[0]))
            ranks = np.zeros((d, 6), dtype=np.int64)
            gammas = np.zeros((d, 2), dtype=np.float64)
            tables = {}
            for f in range(d):
                m = int(count[f])
                if m not in tables:
                    tables[m] = self.column_ranks(m, self.quantile_range)
                ranks[f], gammas[f] = tables[m]
            values = np.zeros((d, 6), dtype=np.float64)
            hip.check(L.tmh_column_select_device(t.x, n, d, hip.ptr(count), hip.ptr(ranks), 6,
                                                 hip.ptr(values), None))
        self.center_, self.scale_ = self.finish(values, gammas)
        self.n_features_in_ = d
        return self

    def _check_fitted(self, d):
        if not hasattr(self, "center_"):
            raise ValueError("This RobustScaler instance is not fitted yet.")
        if d != self.n_features_in_:
            raise ValueError("X has %d features, but RobustScaler is expecting %d features as "
                             "input." % (d, self.n_features_in_))

    def transform(self, X):
        X = as_table(X)
        n, d = X.shape
        self._check_fitted(d)
        out = np.empty_like(X)
        hip.check(hip.lib().tmh_robust_scale(hip.ptr(X), n, d, hip.ptr(self.center_),
                                             hip.ptr(self.scale_), hip.ptr(out)))
        return out

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class KMeans(object):
    """``sklearn.cluster.KMeans`` (Lloyd).  ``init`` is ``'k-means++'`` or an
    array of initial centres; draws come from
    ``numpy.random.RandomState(random_state)`` in scikit-learn's call order
    (``randint`` for the first centre, ``uniform(size=trials)`` per step).
    ``fit(X, scaler=...)`` and ``predict(X, scaler=...)`` scale on load: the
    result is that of ``fit(scaler.transform(X))`` bit for bit, without the
    scaled copy."""

    def __init__(self, n_clusters=8, init="k-means++", n_init=1, max_iter=300, tol=1e-4,
                 random_state=None):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state

    def _check_params(self, X):
        k = self.n_clusters
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("n_clusters must be a positive int, got %r." % (k,))
        if not isinstance(self.n_init, (int, np.integer)) or self.n_init < 1:
            raise ValueError("n_init must be a positive int, got %r." % (self.n_init,))
        if not isinstance(self.max_iter, (int, np.integer)) or self.max_iter < 1:
            raise ValueError("max_iter must be a positive int, got %r." % (self.max_iter,))
        if not self.tol >= 0:
            raise ValueError("tol must not be negative, got %r." % (self.tol,))
        n, d = X.shape
        check_limits(n, d, int(k))
        if n < k:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
        if isinstance(self.init, str):
            if self.init != "k-means++":
                raise ValueError("init must be 'k-means++' or an array of centres, got %r."
                                 % (self.init,))
            return None
        init = np.ascontiguousarray(np.asarray(self.init), dtype=np.float64)
        if init.shape != (k, d):
            raise ValueError("The shape of the initial centers %r does not match (n_clusters, "
                             "n_features) = %r." % (init.shape, (int(k), d)))
        if not np.isfinite(init).all():
            raise ValueError("The initial centers contain NaN or infinity.")
        return init

    @staticmethod
    def _check_finite(X):
        if not np.isfinite(X).all():
            raise ValueError("Input X contains NaN or infinity.")

    @staticmethod
    def n_local_trials(k):
        return 2 + int(np.log(k))

    def _random_state(self):
        if isinstance(self.random_state, np.random.RandomState):
            return self.random_state
        return np.random.RandomState(self.random_state)

    @staticmethod
    def seed(table, k, first, draws, trace=False):
        """k-means++ from given draws [k - 1][trials] on a ``DeviceTable``:
        -> (indices, centres[, trace [k - 1][3 * trials + 1]])."""
        if k > 1:
            draws = np.ascontiguousarray(draws, dtype=np.float64).reshape(k - 1, -1)
            trials = draws.shape[1]
        else:
            trials = 1      # one centre: the first row, no draws
        indices = np.zeros(k, dtype=np.int32)
        centres = np.zeros((k, table.d), dtype=np.float64)
        tr = np.zeros((max(k - 1, 0), 3 * trials + 1), dtype=np.float64) if trace else None
        hip.check(hip.lib().tmh_kmeans_seed_device(
            table.x, table.n, table.d, k, table.center, table.scale, int(first),
            hip.ptr(draws) if k > 1 else None, trials, hip.ptr(indices), hip.ptr(centres),
            hip.ptr_or_null(tr) if (trace and k > 1) else None, None))
        return (indices, centres, tr) if trace else (indices, centres)

    def fit(self, X, y=None, scaler=None):
        X = as_table(X)
        init = self._check_params(X)
        self._check_finite(X)
        n, d = X.shape
        k = int(self.n_clusters)
        if scaler is not None:
            scaler._check_fitted(d)
        rs = self._random_state()
        L = hip.lib()
        best = None
        with DeviceTable(X, scaler) as t:
            dev_labels = t.alloc(4 * n)
            for _ in range(int(self.n_init)):
                if init is None:
                    first = rs.randint(n)
                    trials = self.n_local_trials(k)
                    draws = np.array([rs.uniform(size=trials) for _ in range(k - 1)],
                                     dtype=np.float64).reshape(k - 1, trials)
                    _, start = self.seed(t, k, first, draws)
                else:
                    start = init
                centres = np.zeros((k, d), dtype=np.float64)
                inertia, tol_abs, n_iter = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
                hip.check(L.tmh_kmeans_fit_device(
                    t.x, n, d, k, t.center, t.scale, hip.ptr(start), int(self.max_iter),
                    float(self.tol), hip.ptr(centres), dev_labels, C.byref(inertia),
                    C.byref(n_iter), C.byref(tol_abs), None))
                if best is None or inertia.value < best[0]:
                    labels = dev_labels.get(n, np.int32)
                    hip.check(L.tmh_synchronize(None))
                    best = (inertia.value, centres, labels, n_iter.value, tol_abs.value)
                if init is not None:
                    break   # every run from the same centres is the same run
        self.inertia_, self.cluster_centers_, self.labels_, self.n_iter_, self.tol_abs_ = best
        self.n_features_in_ = d
        return self

    def predict(self, X, scaler=None):
        if not hasattr(self, "cluster_centers_"):
            raise ValueError("This KMeans instance is not fitted yet.")
        X = as_table(X)
        n, d = X.shape
        k = self.cluster_centers_.shape[0]
        if d != self.cluster_centers_.shape[1]:
            raise ValueError("X has %d features, but KMeans is expecting %d features as input."
                             % (d, self.cluster_centers_.shape[1]))
        check_limits(n, d, k)
        self._check_finite(X)
        if scaler is not None:
            scaler._check_fitted(d)
        labels = np.empty(n, dtype=np.int32)
        centres = np.ascontiguousarray(self.cluster_centers_, dtype=np.float64)
        hip.check(hip.lib().tmh_kmeans_predict(
            hip.ptr(X), n, d, k, None if scaler is None else hip.ptr(scaler.center_),
            None if scaler is None else hip.ptr(scaler.scale_), hip.ptr(centres), hip.ptr(labels),
            None))
        return labels

    def fit_predict(self, X, y=None, scaler=None):
        return self.fit(X, scaler=scaler).labels_


class FeatureTable(object):
    """What ``FeatureStore.load_feature_values`` returns: ``values`` [n][d],
    ``index`` (the mapobject ids) and ``columns`` (the feature names), as far as
    the tools read a DataFrame."""

    def __init__(self, values, index, columns):
        self.values = values
        self.index = index
        self.columns = list(columns)

    def __array__(self, dtype=None, copy=None):
        return self.values if dtype is None else self.values.astype(dtype, copy=False)

    def __len__(self):
        return self.values.shape[0]


class FeatureStore(object):
    """In-memory stand-in for the experiment database of the tools, in the
    manner of ``ExperimentStore``: per mapobject type the ids, the feature names
    and the values [n][n_features]."""

    def __init__(self, seed=0):
        self._types = {}
        self.results = {}
        self._rs = np.random.RandomState(seed)

    def add_mapobject_type(self, name, mapobject_ids, feature_names, values):
        ids = np.ascontiguousarray(mapobject_ids, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        if values.shape != (ids.size, len(feature_names)):
            raise ValueError("values must have shape (n_mapobjects, n_features)")
        if np.unique(ids).size != ids.size:
            raise ValueError("mapobject ids must be unique")
        order = np.argsort(ids, kind="stable")
        self._types[name] = (ids[order], list(feature_names), values[order])

    def append_mapobjects(self, name, feature_names, values):
        """Rows for new mapobjects of a type, which is created on first use:
        -> their ids, issued above every existing id of the type, in the order
        of ``values`` [n][n_features].  Feature names other than the type's
        are refused."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        feature_names = list(feature_names)
        if values.ndim != 2 or values.shape[1] != len(feature_names):
            raise ValueError("values must have shape (n_mapobjects, n_features)")
        if name not in self._types:
            old_ids = np.zeros(0, dtype=np.int64)
            old_values = np.zeros((0, len(feature_names)), dtype=np.float64)
        else:
            old_ids, names, old_values = self._types[name]
            if names != feature_names:
                raise ValueError('Feature names differ from those of mapobject type "%s".' % name)
        first = int(old_ids.max()) + 1 if old_ids.size else 1
        ids = np.arange(first, first + values.shape[0], dtype=np.int64)
        self._types[name] = (np.concatenate([old_ids, ids]), feature_names,
                             np.concatenate([old_values, values], axis=0))
        return ids

    def _type(self, name):
        try:
            return self._types[name]
        except KeyError:
            raise ValueError('Unknown mapobject type "%s".' % name)

    def get_random_mapobject_subset(self, mapobject_type_name, n):
        """At most n ids of the type, picked at random (``ORDER BY random() LIMIT n``)."""
        ids = self._type(mapobject_type_name)[0]
        if n >= ids.size:
            return ids[self._rs.permutation(ids.size)]
        return ids[self._rs.choice(ids.size, size=n, replace=False)]

    def partition_mapobjects(self, mapobject_type_name, n):
        """All ids of the type in batches of at most n."""
        if n < 1:
            raise ValueError("batch size must be positive")
        ids = self._type(mapobject_type_name)[0]
        return [ids[i:i + n] for i in range(0, ids.size, n)]

    def load_feature_values(self, mapobject_type_name, feature_names, mapobject_ids=None):
        ids, names, values = self._type(mapobject_type_name)
        cols = []
        for f in feature_names:
            if f not in names:
                raise ValueError('Unknown feature "%s".' % f)
            cols.append(names.index(f))
        if mapobject_ids is None:
            rows = np.arange(ids.size)
        else:
            want = np.asarray(mapobject_ids, dtype=np.int64)
            rows = np.searchsorted(ids, want)
            if (rows >= ids.size).any() or (ids[np.minimum(rows, ids.size - 1)] != want).any():
                raise ValueError("Unknown mapobject id.")
        return FeatureTable(np.ascontiguousarray(values[np.ix_(rows, cols)]), ids[rows],
                            feature_names)

    def register_result(self, submission_id, mapobject_type_name, result_type, **attributes):
        self._type(mapobject_type_name)
        for rid, r in self.results.items():
            if r["submission_id"] == submission_id:
                return rid      # a result may exist already, as in the reference
        rid = len(self.results) + 1
        self.results[rid] = {"submission_id": submission_id, "type": result_type,
                             "mapobject_type": mapobject_type_name, "attributes": attributes,
                             "values": {}}
        return rid

    def save_result_values(self, mapobject_type_name, result_id, data):
        values = self.results[result_id]["values"]
        index = getattr(data, "index", None)
        if index is None:
            raise ValueError("result values need an index of mapobject ids")
        for i, v in zip(np.asarray(index), np.asarray(data)):
            values[int(i)] = int(v)


class Tool(object):
    """tmlib.tools.base.Tool over a ``FeatureStore``."""

    def __init__(self, experiment_id, store=None):
        if store is None:
            raise ValueError("a FeatureStore is required (no database in this build)")
        if not isinstance(store, FeatureStore):
            raise TypeError('Argument "store" must have type FeatureStore.')
        self.experiment_id = experiment_id
        self.store = store

    def get_random_mapobject_subset(self, mapobject_type_name, n):
        return self.store.get_random_mapobject_subset(mapobject_type_name, n)

    def partition_mapobjects(self, mapobject_type_name, n):
        return self.store.partition_mapobjects(mapobject_type_name, n)

    def load_feature_values(self, mapobject_type_name, feature_names, mapobject_ids=None):
        return self.store.load_feature_values(mapobject_type_name, feature_names, mapobject_ids)

    def register_result(self, submission_id, mapobject_type_name, result_type,
                        **result_attributes):
        return self.store.register_result(submission_id, mapobject_type_name, result_type,
                                          **result_attributes)

    def save_result_values(self, mapobject_type_name, result_id, data):
        return self.store.save_result_values(mapobject_type_name, result_id, data)

    def process_request(self, submission_id, payload):
        raise NotImplementedError


class Classifier(Tool):
    """Abstract base class for classification tools."""

    def train_supervised(self, feature_data, labels, method, n_fold_cv):
        raise NotSupportedError("Supervised classification (random forest, SVM, logistic "
                                "regression with grid search) is not built.")

    def train_unsupervised(self, feature_data, k, method):
        """-> (model, scaler), trained on ``feature_data`` (base.py:586-619)."""
        classifiers = {
            "kmeans": {"cls": KMeans, "scaler": RobustScaler(quantile_range=(1.0, 99.0))}
        }
        if method not in classifiers:
            raise ValueError('Unknown method "%s".' % method)
        logger.info('train "%s" classifier for %d classes', method, k)
        scaler = classifiers[method]["scaler"]
        X = as_table(feature_data)
        if scaler:
            scaler.fit(X)
        model = classifiers[method]["cls"](n_clusters=k)
        model.fit(X, scaler=scaler if scaler else None)   # scaled on load
        return (model, scaler)

    def predict(self, feature_data, model, scaler=None):
        """Labels of ``feature_data`` (base.py:621-645): a pandas Series when the
        input had an ``.index``, else an array."""
        logger.info("predict labels")
        predictions = model.predict(as_table(feature_data), scaler=scaler)
        index = getattr(feature_data, "index", None)
        if index is None:
            return predictions
        import pandas as pd
        return pd.Series(predictions, index=index)
