"""GPU: the supervised classification tool against the
recorded scikit-learn results and the numpy literal.

Comparison rules.  Forest labels and probabilities are scikit-learn's exactly
(``array_equal``): the rule is adds in a fixed order and one divide.  An SVC
row is *close* when some pair's decision value lies within
64 (d + m_pair) 2^-52 (sum |coef_s| A_s + |rho|) of zero
(classification_literal.svc_predict); labels must agree on every other row and
at most 0.1 % of a case's rows may be close (the golden generator asserts that
the literal meets none, so the allowance is a condition, not a tolerance);
decision values agree with ``decision_function(..., 'ovo')`` in libsvm's sign
within the same bound.  Routes (LDS / memory, one tile / streamed) and repeated
runs give identical bytes.
"""

import numpy as np
import pytest

import classification_cases as cases
import classification_literal as lit
from test_classification_cpu import big_forest, create_forest, golden, scaled_table, svc_literal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


def forest_of(model):
    from tmlibrary_amd.tools import ForestModel
    return ForestModel.from_arrays(**model)


def svc_of(model):
    from tmlibrary_amd.tools import SVCModel
    return SVCModel.from_arrays(**model)


def scaler_of(rest):
    from tmlibrary_amd.tools.base import RobustScaler
    if "center" not in rest:
        return None
    s = RobustScaler()
    s.center_, s.scale_, s.n_features_in_ = rest["center"], rest["scale"], rest["X"].shape[1]
    return s


def forest_device(L, model, X, want_proba=True, skip=0):
    """tmh_forest_predict_device on a table in device memory, from row `skip`
    on -> (labels, proba)"""
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import DeviceTable
    n, c = X.shape[0] - skip, model.classes_.size
    proba = None
    with DeviceTable(X) as t:
        d_labels = t.alloc(4 * n)
        d_proba = t.alloc(8 * n * c) if want_proba else None
        x = t.x.at(8 * skip * X.shape[1])
        hip.check(L.tmh_forest_predict_device(model.handle(), x, n, d_labels, d_proba, None))
        labels = d_labels.get(n, np.int32)
        if want_proba:
            proba = d_proba.get((n, c), np.float64)
        hip.check(L.tmh_synchronize(None))
    return labels, proba


def svc_device(L, model, X, scaler, want_dec=True):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import DeviceTable
    n, pairs = X.shape[0], model.rho.size
    dec = None
    with DeviceTable(X, scaler) as t:
        d_labels = t.alloc(4 * n)
        d_dec = t.alloc(8 * n * pairs) if want_dec else None
        hip.check(L.tmh_svc_predict_device(model.handle(), t.x, n, t.center, t.scale, d_labels,
                                           d_dec, None))
        labels = d_labels.get(n, np.int32)
        if want_dec:
            dec = d_dec.get((n, pairs), np.float64)
        hip.check(L.tmh_synchronize(None))
    return labels, dec


def assert_svc(name, labels, dec, rows=slice(None)):
    """labels equal outside the close rows (at most 0.1 %), dec within the bound"""
    _, rest = golden(name)
    _, _, close, bound = svc_literal(name)
    close, bound = close[rows], bound[rows]
    assert close.sum() <= close.size // 1000
    bad = np.flatnonzero((labels != rest["labels"][rows]) & ~close)
    assert bad.size == 0, "%d labels differ, first at row %d" % (bad.size, bad[0])
    if dec is not None:
        assert (np.abs(dec - rest["dec"][rows]) <= bound).all()


# ---- forest ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.FOREST_GOLDEN)
def test_forest_equals_sklearn_on_both_routes(L, name):
    arrays, rest = golden(name)
    model = forest_of(arrays)
    assert model.route()[0] == "lds"
    proba = model.predict_proba(rest["X"])
    assert np.array_equal(proba, rest["proba"])
    assert np.array_equal(model.predict(rest["X"]), arrays["classes"][rest["labels"]])
    assert model.predict_proba(rest["X"]).tobytes() == proba.tobytes()       # a second run
    d_labels, d_proba = forest_device(L, model, rest["X"])
    assert np.array_equal(d_labels, rest["labels"]) and d_proba.tobytes() == proba.tobytes()
    assert np.array_equal(forest_device(L, model, rest["X"], want_proba=False)[0], rest["labels"])
    model.memory_route = True
    assert model.route() == ("memory", model.route()[1])
    assert model.predict_proba(rest["X"]).tobytes() == proba.tobytes()
    m_labels, m_proba = forest_device(L, model, rest["X"])
    assert np.array_equal(m_labels, rest["labels"]) and m_proba.tobytes() == proba.tobytes()


@pytest.mark.parametrize("name,tile", [("forest_d7_c5_t3", 256), ("forest_d33_c2_t24", 170)])
def test_forest_rows_around_the_tile(L, name, tile):
    """n = 1 and n one below, at and one above the row tile, on both routes"""
    arrays, rest = golden(name)
    spec = cases.FOREST_GOLDEN[name]
    assert tile == min(256, 8192 // (spec["d"] | 1), 4096 // spec["classes"],
                       4096 // arrays["tree_root"].size)
    model = forest_of(arrays)
    for memory in (False, True):
        model.memory_route = memory
        for n in (1, tile - 1, tile, tile + 1):
            X = np.ascontiguousarray(rest["X"][:n])
            assert np.array_equal(model.predict_proba(X), rest["proba"][:n]), (memory, n)
        # a table that starts on an odd element: the 8-byte loads of an unaligned tile
        assert spec["d"] % 2 == 1
        labels, proba = forest_device(L, model, rest["X"][:tile + 2], skip=1)
        assert np.array_equal(proba, rest["proba"][1:tile + 2])
        assert np.array_equal(labels, rest["labels"][1:tile + 2])


def test_forest_constructed_cases(L):
    for build in (cases.threshold_case, cases.tie_case, lambda: cases.divide_case()[:2]):
        arrays, X = build()
        labels, proba = lit.forest_predict(arrays, X)
        model = forest_of(arrays)
        for memory in (False, True):
            model.memory_route = memory
            assert np.array_equal(model.predict_proba(X), proba)
            assert np.array_equal(model.predict(X), arrays["classes"][labels])
    # f64 just above a threshold, f32 on it: left (an f64 compare would go right)
    arrays, X = cases.threshold_case()
    assert np.array_equal(forest_of(arrays).predict(X)[:3], [0.0, 0.0, 0.0])
    # the exact tie goes to the first class; the divide merges two unequal sums into a tie
    assert np.array_equal(forest_of(cases.tie_case()[0]).predict(cases.tie_case()[1]), [0.0] * 3)
    assert np.array_equal(forest_of(cases.divide_case()[0]).predict(cases.divide_case()[1]), [0.0] * 2)


def test_big_forest_takes_the_memory_route_by_itself(L):
    arrays, X, (labels, proba) = big_forest()
    model = forest_of(arrays)
    route, nodes = model.route()
    assert route == "memory" and nodes == arrays["feature"].size > 6144
    got = model.predict_proba(X)
    assert np.array_equal(got, proba) and np.array_equal(model.predict(X), arrays["classes"][labels])
    d_labels, d_proba = forest_device(L, model, X)
    assert np.array_equal(d_labels, labels) and d_proba.tobytes() == got.tobytes()


def test_forest_refusals(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import DeviceTable
    for name, arrays in cases.malformed_forests().items():
        rc, h = create_forest(L, arrays)
        assert rc == hip.TMH_EINVAL and not h.value, name
    model = forest_of(cases.small_forest())
    h = model.handle()
    X = np.zeros((5, 3))
    for bad, text in ((np.nan, b"NaN or infinite"), (np.inf, b"NaN or infinite"),
                      (3.5e38, b"too large for float32"), (-1e300, b"too large for float32")):
        X[3, 1] = bad
        labels = np.zeros(5, np.int32)
        assert L.tmh_forest_predict(h, hip.ptr(X), 5, hip.ptr(labels), None) == hip.TMH_EINVAL
        assert text in L.tmh_last_error()
    X[3, 1] = lit.F32_MAX       # the largest float32 itself is data
    assert L.tmh_forest_predict(h, hip.ptr(X), 5, hip.ptr(labels), None) == hip.TMH_OK
    with DeviceTable(X) as t:
        out = t.alloc(8 * 5 * 2)
        # x overlapping an output, NULL pointers, and row counts past the limit
        assert L.tmh_forest_predict_device(h, t.x, 5, t.x, None, None) == hip.TMH_EINVAL
        assert b"overlap" in L.tmh_last_error()
        assert L.tmh_forest_predict_device(h, t.x, 5, out, t.x, None) == hip.TMH_EINVAL
        assert L.tmh_forest_predict_device(h, t.x, 5, None, None, None) == hip.TMH_EINVAL
        # labels overlapping the probabilities: both are written by one kernel
        assert L.tmh_forest_predict_device(h, t.x, 5, out, out, None) == hip.TMH_EINVAL
        assert b"outputs must not overlap" in L.tmh_last_error()
        assert L.tmh_forest_predict_device(h, t.x, 5, out.at(16), out, None) \
            == hip.TMH_EINVAL
        assert L.tmh_forest_predict_device(h, t.x, 0, out, None, None) == hip.TMH_EINVAL
        assert L.tmh_forest_predict_device(h, t.x, 2 ** 31, out, None, None) == hip.TMH_EINVAL
        assert b"2^31" in L.tmh_last_error()
    assert L.tmh_forest_set_option(h, 99, 1) == hip.TMH_EINVAL
    assert L.tmh_forest_set_option(h, hip.TMH_OPT_FOREST_MEMORY_ROUTE, 2) == hip.TMH_EINVAL
    model.close()
    assert model._handle is None


# ---- SVC -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.SVC_GOLDEN)
def test_svc_equals_sklearn_on_both_routes(L, name):
    arrays, rest = golden(name)
    model, scaler, X = svc_of(arrays), scaler_of(rest), rest["X"]
    tile, tiles = model.tile()
    dec = model.decision_function(X, scaler=scaler)
    labels = model.predict(X, scaler=scaler)
    assert_svc(name, np.searchsorted(arrays["classes"], labels), dec)
    assert model.decision_function(X, scaler=scaler).tobytes() == dec.tobytes()     # a second run
    d_labels, d_dec = svc_device(L, model, X, scaler)
    assert d_dec.tobytes() == dec.tobytes()
    assert np.array_equal(arrays["classes"][d_labels], labels)
    assert np.array_equal(svc_device(L, model, X, scaler, want_dec=False)[0], d_labels)
    # the streamed route: a tile of 5 support vectors
    model.tile_cap = 5
    rows = arrays["sv"].shape[0] if str(arrays["kernel"]) == "rbf" else arrays["rho"].size
    assert model.tile() == (min(5, tile), -(-rows // min(5, tile)))
    assert model.decision_function(X, scaler=scaler).tobytes() == dec.tobytes()
    s_labels, s_dec = svc_device(L, model, X, scaler)
    assert s_dec.tobytes() == dec.tobytes() and np.array_equal(s_labels, d_labels)


def test_svc_rows_around_the_tile(L):
    name, tile = "svc_rbf_d7_k3", 256
    arrays, rest = golden(name)
    assert tile == max(4, min(256, 4096 // 7, 2048 // 3) & ~3)
    model, scaler = svc_of(arrays), scaler_of(rest)
    full = model.decision_function(rest["X"], scaler=scaler)
    for n in (1, tile - 1, tile, tile + 1):
        rows = slice(0, n)
        dec = model.decision_function(rest["X"][rows], scaler=scaler)
        labels = model.predict(rest["X"][rows], scaler=scaler)
        assert_svc(name, np.searchsorted(arrays["classes"], labels), dec, rows)
        assert dec.tobytes() == full[rows].tobytes()    # a row's values do not depend on its tile


@pytest.mark.parametrize("name", ["svc_rbf_d33_k5", "svc_linear_d7_k5"])
def test_scaling_on_load_equals_the_scaled_table(L, name):
    arrays, rest = golden(name)
    model, scaler = svc_of(arrays), scaler_of(rest)
    Xs = scaler.transform(rest["X"])        # tmh_robust_scale
    assert np.array_equal(Xs, scaled_table(rest))
    on_load = model.decision_function(rest["X"], scaler=scaler)
    assert model.decision_function(Xs).tobytes() == on_load.tobytes()
    assert np.array_equal(model.predict(Xs), model.predict(rest["X"], scaler=scaler))


def test_svc_refusals(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import DeviceTable
    model = svc_of(cases.small_svc())
    h = model.handle()
    X = np.zeros((4, 2))
    labels = np.zeros(4, np.int32)
    center, scale = np.zeros(2), np.ones(2)
    for bad in (np.nan, -np.inf):
        X[1, 1] = bad
        assert L.tmh_svc_predict(h, hip.ptr(X), 4, None, None, hip.ptr(labels), None) \
            == hip.TMH_EINVAL
        assert b"NaN or infinite" in L.tmh_last_error()
    X[1, 1] = 0.5
    assert L.tmh_svc_predict(h, hip.ptr(X), 4, hip.ptr(center), None, hip.ptr(labels), None) \
        == hip.TMH_EINVAL       # center without scale
    with DeviceTable(X) as t:
        out = t.alloc(8 * 4 * 3)
        assert L.tmh_svc_predict_device(h, t.x, 4, None, None, t.x, None, None) == hip.TMH_EINVAL
        assert b"overlap" in L.tmh_last_error()
        assert L.tmh_svc_predict_device(h, t.x, 4, None, None, out, t.x, None) == hip.TMH_EINVAL
        assert L.tmh_svc_predict_device(h, t.x, 4, None, None, None, None, None) == hip.TMH_EINVAL
        assert L.tmh_svc_predict_device(h, t.x, 4, None, None, out, out, None) == hip.TMH_EINVAL
        assert b"outputs must not overlap" in L.tmh_last_error()
        assert L.tmh_svc_predict_device(h, t.x, 2 ** 31, None, None, out, None, None) \
            == hip.TMH_EINVAL
    assert L.tmh_svc_set_option(h, hip.TMH_OPT_SVC_TILE, -1) == hip.TMH_EINVAL
    assert L.tmh_svc_set_option(h, 99, 1) == hip.TMH_EINVAL
    # the small model against the literal, rbf and linear
    rs = np.random.RandomState(8)
    X = rs.normal(0.0, 2.0, size=(300, 2))
    for kernel in ("rbf", "linear"):
        arrays = cases.small_svc(kernel)
        want, dec, close = lit.svc_predict(arrays, X)
        m = svc_of(arrays)
        got = m.decision_function(X)
        assert (np.abs(got - dec) <= lit.svc_dec_bound(arrays, X)).all()
        assert not close.any() and np.array_equal(m.predict(X), arrays["classes"][want])


# ---- the tool, end to end ---------------------------------------------------------------

def store_of(rest, n_features):
    from tmlibrary_amd.tools.base import FeatureStore
    store = FeatureStore(seed=1)
    n = rest["X"].shape[0]
    ids = 1000 + np.arange(n)
    store.add_mapobject_type("Cells", ids, ["f%d" % i for i in range(n_features)], rest["X"])
    return store, ids


@pytest.mark.parametrize("method,name", [("randomforest", "forest_d7_c5_t3"),
                                         ("svm", "svc_rbf_d7_k3")])
def test_process_request_end_to_end(L, method, name):
    """the model comes from a golden: the labelling of every object runs on the
    GPU in batches, without scikit-learn"""
    from tmlibrary_amd.tools import Classification
    arrays, rest = golden(name)
    store, ids = store_of(rest, 7)
    tool = Classification(1, store=store)
    tool.n_test = 500       # three batches, the last one short
    model = forest_of(arrays) if method == "randomforest" else svc_of(arrays)
    tool.train_supervised = lambda *a, **k: (model, scaler_of(rest))
    classes = [{"name": "class %d" % c, "object_ids": [int(i) for i in ids[c * 10:c * 10 + 10]],
                "color": "#%06x" % c} for c in range(arrays["classes"].size)]
    rid = tool.process_request(3, {"chosen_object_type": "Cells",
                                   "selected_features": ["f%d" % i for i in range(7)],
                                   "training_classes": classes,
                                   "options": {"method": method, "n_fold_cv": 3}})
    values = store.results[rid]["values"]
    got = np.array([values[int(i)] for i in ids])
    if method == "svm":
        assert_svc(name, got, None)
    else:
        assert np.array_equal(got, rest["labels"])
    assert store.results[rid]["type"] == "SupervisedClassifierToolResult"
    assert np.array_equal(store.results[rid]["attributes"]["unique_labels"],
                          np.arange(arrays["classes"].size, dtype=np.float64))


@pytest.mark.parametrize("method", ["randomforest", "svm"])
def test_process_request_trains_for_real(L, method):
    pytest.importorskip("sklearn")
    from tmlibrary_amd.tools import Classification
    from tmlibrary_amd.tools.base import FeatureStore
    rs = np.random.RandomState(6)
    n = 3000
    truth = rs.randint(2, size=n)
    X = rs.normal(0.0, 1.0, size=(n, 4)) + 4.0 * truth[:, None]
    store = FeatureStore(seed=2)
    ids = 10 + np.arange(n)
    store.add_mapobject_type("Cells", ids, list("abcd"), X)
    tool = Classification(1, store=store)
    tool.n_test = 1024
    train = rs.permutation(n)[:40]      # interleaved, so that every fold sees both classes
    classes = [{"name": str(c), "color": "#000000",
                "object_ids": [int(ids[i]) for i in train if truth[i] == c]} for c in (0, 1)]
    rid = tool.process_request(9, {"chosen_object_type": "Cells",
                                   "selected_features": list("abcd"),
                                   "training_classes": classes,
                                   "options": {"method": method, "n_fold_cv": 2,
                                               "random_state": 0}})
    values = store.results[rid]["values"]
    got = np.array([values[int(i)] for i in ids])
    assert (got == truth).mean() > 0.97
