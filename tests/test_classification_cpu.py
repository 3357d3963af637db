"""CPU: the supervised classification tool's rules and its Python layer
(DESIGN.md section 23).

The numpy literal (tests/classification_literal.py) equals the recorded
scikit-learn results (tests/golden/classification_*.npz): forests bit for bit,
SVCs without a close row.  tmlibrary_amd/csrc/classify_core.h -- the validator,
the packing, the row walk and the pair accumulation the kernels run -- is
compiled with g++ through tests/classify_host.cpp, plainly and under
AddressSanitizer and UBSan, and agrees with the literal on the goldens, the
constructed forests and the malformed models.  The exporter, the models'
argument checks, the C-ABI's refusal of malformed models and the tool's payload
handling need no GPU.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import classification_cases as cases
import classification_literal as lit
from util import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
HARNESS = os.path.join(REPO, "tests", "classify_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]


@functools.lru_cache(maxsize=None)
def golden(name):
    """-> (model arrays, the other arrays) of a golden case"""
    with np.load(os.path.join(GOLDEN, "classification_%s.npz" % name)) as z:
        model = {k[2:]: z[k] for k in z.files if k.startswith("m_")}
        rest = {k: z[k] for k in z.files if not k.startswith("m_")}
    return model, rest


def scaled_table(rest):
    return lit.scale(rest["X"], rest["center"], rest["scale"]) if "center" in rest else rest["X"]


@functools.lru_cache(maxsize=None)
def svc_literal(name):
    """the literal's (labels, dec, close, bound) of a golden SVC case, computed once"""
    model, rest = golden(name)
    Xs = scaled_table(rest)
    return lit.svc_predict(model, Xs) + (lit.svc_dec_bound(model, Xs),)


@functools.lru_cache(maxsize=None)
def big_forest():
    model, X = cases.big_forest()
    return model, X, lit.forest_predict(model, X)


# ---- the literal against the goldens ----------------------------------------------------

@pytest.mark.parametrize("name", cases.FOREST_GOLDEN)
def test_forest_literal_equals_golden(name):
    model, rest = golden(name)
    assert lit.forest_validate(model) is None
    labels, proba = lit.forest_predict(model, rest["X"])
    assert proba.tobytes() == rest["proba"].tobytes()
    assert np.array_equal(labels, rest["labels"])
    spec = cases.FOREST_GOLDEN[name]
    assert rest["X"].shape == (spec["n"], spec["d"]) and proba.shape[1] == spec["classes"]


def test_single_leaf_tree_is_in_its_golden():
    model, _ = golden("forest_d1_c16_leaf")
    at = cases.FOREST_GOLDEN["forest_d1_c16_leaf"]["single_leaf_at"]
    assert model["feature"][model["tree_root"][at]] == -1
    assert model["tree_root"][at + 1] == model["tree_root"][at] + 1


@pytest.mark.parametrize("name", cases.SVC_GOLDEN)
def test_svc_literal_equals_golden(name):
    model, rest = golden(name)
    labels, dec, close, bound = svc_literal(name)
    assert close.sum() == 0                 # the condition the 0.1 % allowance rests on
    assert np.array_equal(labels, rest["labels"])
    assert (np.abs(dec - rest["dec"]) <= bound).all()
    spec = cases.SVC_GOLDEN[name]
    assert str(model["kernel"]) == spec["kernel"] and ("center" in rest) == spec["scaler"]


def test_constructed_cases_are_what_they_say():
    model, X = cases.threshold_case()
    leaves = lit.forest_leaves(model, X)
    value = model["leaf_value"]
    # f64 just above the threshold, f32 equal to it: left, where an f64 compare goes right
    assert X[1, 0] > cases.F32_THRESHOLD and np.float32(X[1, 0]) == np.float32(cases.F32_THRESHOLD)
    assert np.array_equal(value[leaves[0, 0]], [1, 0]) and np.array_equal(value[leaves[1, 0]], [1, 0])
    assert np.array_equal(value[leaves[4, 0]], [0, 1])
    assert np.array_equal(value[leaves[5, 1]], [0.25, 0.75]) and \
        np.array_equal(value[leaves[6, 1]], [0.25, 0.75])
    labels, proba = lit.forest_predict(model, X)
    in_f64 = X[:, 0] <= cases.F32_THRESHOLD
    assert not in_f64[1] and not in_f64[2]      # a kernel comparing in f64 fails rows 1 and 2
    model, X = cases.tie_case()
    labels, proba = lit.forest_predict(model, X)
    assert np.array_equal(proba, [[0.5, 0.5, 0.0]] * 3) and np.array_equal(labels, [0, 0, 0])
    model, X, a, b = cases.divide_case()
    assert a < b and a / 3.0 == b / 3.0
    labels, proba = lit.forest_predict(model, X)
    assert np.array_equal(labels, [0, 0]) and proba[0, 0] == proba[0, 1]
    model, X, _ = big_forest()
    assert lit.forest_validate(model) is None
    assert model["feature"].size * 16 > 96 * 1024      # beyond the LDS route's 96 KB


def test_malformed_models_are_refused_by_the_literal():
    assert lit.forest_validate(cases.small_forest()) is None
    for name, model in cases.malformed_forests().items():
        assert lit.forest_validate(model) is not None, name


# ---- classify_core.h on the host --------------------------------------------------------

def forest_record(model, X):
    f = model
    head = [np.array([0], np.int32), np.array([f["feature"].size], np.int64),
            np.array([f["tree_root"].size], np.int32), np.array([f["leaf_value"].shape[0]], np.int64),
            np.array([f["leaf_value"].shape[1], int(f["n_features"])], np.int32),
            np.array([X.shape[0]], np.int64)]
    body = [f["feature"].astype(np.int32), f["threshold"].astype(np.float64),
            f["left"].astype(np.int32), f["right"].astype(np.int32), f["leaf_row"].astype(np.int32),
            f["tree_root"].astype(np.int32), f["leaf_value"].astype(np.float64),
            np.ascontiguousarray(X, np.float64)]
    return b"".join(a.tobytes() for a in head + body)


def svc_record(model, X, center=None, scale=None, tile=0):
    s = model
    m, d = s["sv"].shape
    head = [np.array([1, 0 if str(s["kernel"]) == "rbf" else 1], np.int32),
            np.array([float(s["gamma"])], np.float64), np.array([m], np.int64),
            np.array([d, s["n_sv"].size, center is not None, tile], np.int32),
            np.array([X.shape[0]], np.int64)]
    body = [s["sv"].astype(np.float64), s["n_sv"].astype(np.int32), s["coef"].astype(np.float64),
            s["rho"].astype(np.float64)]
    if center is not None:
        body += [np.asarray(center, np.float64), np.asarray(scale, np.float64)]
    body.append(np.ascontiguousarray(X, np.float64))
    return b"".join(a.tobytes() for a in head + body)


def run_host(exe, tmp_path, records):
    """[(bytes, n, columns)] -> [(status, labels, values)]"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(np.array([len(records)], np.int32).tobytes())
        for raw, _, _ in records:
            f.write(raw)
    subprocess.run([exe, src, dst], check=True)
    raw, at, out = open(dst, "rb").read(), 0, []
    for _, n, cols in records:
        status = int(np.frombuffer(raw, np.int32, 1, at)[0])
        at += 4
        if status != 0:
            out.append((status, None, None))
            continue
        labels = np.frombuffer(raw, np.int32, n, at)
        at += 4 * n
        values = np.frombuffer(raw, np.float64, n * cols, at).reshape(n, cols)
        at += 8 * n * cols
        out.append((status, labels, values))
    assert at == len(raw)
    return out


def host_records():
    """every record the host program runs, with what the literal says of it"""
    records, expect = [], []
    for name in cases.FOREST_GOLDEN:
        model, rest = golden(name)
        records.append((forest_record(model, rest["X"]), rest["X"].shape[0], rest["proba"].shape[1]))
        expect.append(("forest", name, rest["labels"], rest["proba"]))
    for build in (cases.threshold_case, cases.tie_case, lambda: cases.divide_case()[:2]):
        model, X = build()
        labels, proba = lit.forest_predict(model, X)
        records.append((forest_record(model, X), X.shape[0], proba.shape[1]))
        expect.append(("forest", "constructed", labels, proba))
    model, X, (labels, proba) = big_forest()
    records.append((forest_record(model, X), X.shape[0], proba.shape[1]))
    expect.append(("forest", "big", labels, proba))
    for name, model in cases.malformed_forests().items():
        records.append((forest_record(model, np.zeros((1, 3))), 1, 2))
        expect.append(("refused", name, 1, None))
    for bad in (np.nan, np.inf, 3.5e38, -1e300):
        X = np.zeros((2, 3))
        X[1, 2] = bad
        assert lit.forest_refuses(X)
        records.append((forest_record(cases.small_forest(), X), 2, 2))
        expect.append(("refused", "x = %r" % bad, 2, None))
    # the largest finite float32, and a value that rounds down to it: taken
    X = np.array([[lit.F32_MAX, 0.0, 0.0], [3.4028235e38, 1.0, -1.0]])
    assert not lit.forest_refuses(X)
    labels, proba = lit.forest_predict(cases.small_forest(), X)
    records.append((forest_record(cases.small_forest(), X), 2, 2))
    expect.append(("forest", "f32 max", labels, proba))
    for name in cases.SVC_GOLDEN:
        model, rest = golden(name)
        labels, dec, _, bound = svc_literal(name)
        for tile in (0, 7):
            records.append((svc_record(model, rest["X"], rest.get("center"), rest.get("scale"), tile),
                            rest["X"].shape[0], dec.shape[1]))
            expect.append(("svc", name, labels, (dec, bound)))
    bad = dict(cases.small_svc(), n_sv=np.array([2, 2, 2], np.int32))
    records.append((svc_record(bad, np.zeros((1, 2))), 1, 3))
    expect.append(("refused", "n_sv", 1, None))
    return records, expect


def check_host(exe, tmp_path):
    records, expect = host_records()
    got = run_host(exe, tmp_path, records)
    tiled = {}
    for (status, labels, values), (kind, name, want, more) in zip(got, expect):
        if kind == "refused":
            assert status == want, name
            continue
        assert status == 0, name
        assert np.array_equal(labels, want), name
        if kind == "forest":
            assert values.tobytes() == more.tobytes(), name
        else:
            dec, bound = more
            assert (np.abs(values - dec) <= bound).all(), name
            # walking the support vectors in tiles of 7 gives the bytes of one pass
            assert tiled.setdefault(name, values.tobytes()) == values.tobytes(), name


def test_core_on_the_host(tmp_path):
    exe = str(tmp_path / "classify_host")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", exe, HARNESS], check=True, capture_output=True)
    check_host(exe, tmp_path)


def test_core_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "classify_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                   + FLAGS + ["-o", exe, HARNESS], check=True, capture_output=True)
    check_host(exe, tmp_path)


# ---- the exporter -----------------------------------------------------------------------

def test_exporter_round_trip():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.svm import SVC
    from tmlibrary_amd.tools import ForestModel, SVCModel
    spec = cases.FOREST_GOLDEN["forest_d7_c5_t3"]
    Xt, y = cases.training_set(spec)
    rf = RandomForestClassifier(n_estimators=3, max_depth=3, random_state=spec["seed"]).fit(Xt, y)
    model = ForestModel.from_sklearn(rf)
    again = ForestModel.from_arrays(**model.to_arrays())
    recorded, _ = golden("forest_d7_c5_t3")
    for key, value in again.to_arrays().items():
        assert np.array_equal(value, model.to_arrays()[key]), key
        assert np.array_equal(value, recorded[key]), key        # the golden is this export
    assert lit.forest_validate(again.to_arrays()) is None
    assert np.array_equal(again.classes_, rf.classes_) and again.n_features_in_ == 7
    X = cases.table(spec)[:50]
    assert lit.forest_predict(again.to_arrays(), X)[1].tobytes() == rf.predict_proba(X).tobytes()
    # libsvm's own sign: for two classes scikit-learn's public attributes are flipped
    spec = cases.SVC_GOLDEN["svc_rbf_d1_k2"]
    Xt, y = cases.training_set(spec)
    svc = SVC(kernel="rbf", C=spec["C"], gamma=spec["gamma"]).fit(Xt, y)
    model = SVCModel.from_arrays(**SVCModel.from_sklearn(svc).to_arrays())
    assert np.array_equal(model.coef, svc._dual_coef_) and np.array_equal(model.coef, -svc.dual_coef_)
    assert np.array_equal(model.rho, -svc._intercept_) and np.array_equal(model.rho, svc.intercept_)
    assert model.gamma == svc._gamma and model.kernel == "rbf"
    X = cases.table(spec)[:50]
    labels, dec, close = lit.svc_predict(model.to_arrays(), X)
    assert not close.any() and np.array_equal(svc.classes_[labels], svc.predict(X))
    assert np.allclose(dec[:, 0], -svc.decision_function(X), rtol=0, atol=1e-9)


def test_train_supervised_returns_flat_models():
    pytest.importorskip("sklearn")
    from tmlibrary_amd.tools import ForestModel, SVCModel, train_supervised
    from tmlibrary_amd.tools.base import FeatureTable, RobustScaler
    rs = np.random.RandomState(4)
    X = np.concatenate([rs.normal(0.0, 1.0, (30, 3)), rs.normal(3.0, 1.0, (30, 3))])
    order = rs.permutation(60)
    ids = np.arange(500, 560)
    labels = {int(i): float(c) for i, c in zip(ids, (order >= 30))}
    data = FeatureTable(X[order], ids, ["a", "b", "c"])
    model, scaler = train_supervised(data, labels, "svm", 3)
    assert isinstance(model, SVCModel) and isinstance(scaler, RobustScaler)
    assert np.array_equal(scaler.center_, np.median(X, axis=0)) and model.n_features_in_ == 3
    assert np.array_equal(model.classes_, [0.0, 1.0])
    got, _, _ = lit.svc_predict(model.to_arrays(), lit.scale(X[order], scaler.center_, scaler.scale_))
    assert (got == (order >= 30)).mean() > 0.9
    with pytest.raises(ValueError, match='Unknown method "boosting".'):
        train_supervised(data, labels, "boosting", 3)
    with pytest.raises(ValueError, match="index"):
        train_supervised(X, labels, "svm", 3)


# ---- the models' argument checks -------------------------------------------------------

def test_limits_are_refused_by_name():
    from tmlibrary_amd.tools import ForestModel, SVCModel
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    ok = cases.small_forest()
    assert ForestModel.from_arrays(**ok).n_features_in_ == 3

    def forest(**changes):
        return ForestModel.from_arrays(**dict(ok, **changes))

    with pytest.raises(NotSupportedError, match="at most 256"):
        forest(n_features=257)
    with pytest.raises(NotSupportedError, match="2 to 64 classes"):
        forest(classes=np.arange(65.0), leaf_value=np.zeros((5, 65)))
    with pytest.raises(NotSupportedError, match="2 to 64 classes"):
        forest(classes=np.arange(1.0), leaf_value=np.zeros((5, 1)))
    with pytest.raises(NotSupportedError, match="1 to 256 trees"):
        forest(tree_root=np.arange(257))
    big = {k: np.zeros(2 ** 24, t) for k, t in (
        ("feature", np.int8), ("threshold", np.float16), ("left", np.int8), ("right", np.int8),
        ("leaf_row", np.int8))}
    with pytest.raises(NotSupportedError, match="fewer than 2\\*\\*24 nodes"):
        forest(**big)       # 2^24 nodes, one over; the arrays are converted after the check
    with pytest.raises(ValueError, match="one entry per node"):
        forest(left=ok["left"][:-1])
    with pytest.raises(ValueError, match="n_leaves, n_classes"):
        forest(leaf_value=np.zeros((5, 3)))
    sv = cases.small_svc()

    def svc(**changes):
        return SVCModel.from_arrays(**dict(sv, **changes))

    assert svc().n_features_in_ == 2
    with pytest.raises(NotSupportedError, match='"rbf" and "linear"'):
        svc(kernel=np.str_("poly"))
    with pytest.raises(NotSupportedError, match="2 to 16 classes"):
        svc(classes=np.arange(17.0))
    with pytest.raises(NotSupportedError, match="at most 256"):
        svc(sv=np.zeros((5, 257)))
    with pytest.raises(NotSupportedError, match="1 to 65536"):
        svc(sv=np.zeros((65537, 2)))
    with pytest.raises(ValueError, match="shapes"):
        svc(rho=np.zeros(2))


def test_refused_input_needs_no_gpu():
    from tmlibrary_amd.tools import ForestModel, SVCModel
    forest = ForestModel.from_arrays(**cases.small_forest())
    svc = SVCModel.from_arrays(**cases.small_svc())
    X = np.zeros((4, 3))
    for bad, what in ((np.nan, "NaN"), (-np.inf, "infinity"), (3.5e38, "float32")):
        X[2, 1] = bad
        with pytest.raises(ValueError, match=what):
            forest.predict(X)
    with pytest.raises(ValueError, match="expecting 3 features"):
        forest.predict(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="2D"):
        forest.predict(np.zeros(3))
    with pytest.raises(ValueError, match="NaN"):
        svc.predict(np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError, match="expecting 2 features"):
        svc.decision_function(np.zeros((4, 3)))


# ---- the C-ABI ----------------------------------------------------------------------------

def test_abi_agreement_covers_the_new_symbols():
    from tmlibrary_amd import hip
    text = open(os.path.join(REPO, "include", "tmhip.h")).read()
    lib = hip.load_library()
    names = ["tmh_%s_%s" % (a, b) for a in ("forest", "svc")
             for b in ("create", "destroy", "set_option", "predict", "predict_device")]
    for name in names + ["tmh_forest_route", "tmh_svc_tile"]:
        assert name in hip.SIGNATURES and name + "(" in text and hasattr(lib, name), name
    for name, value in (("TMH_OPT_FOREST_MEMORY_ROUTE", hip.TMH_OPT_FOREST_MEMORY_ROUTE),
                        ("TMH_OPT_SVC_TILE", hip.TMH_OPT_SVC_TILE),
                        ("TMH_SVC_RBF", hip.TMH_SVC_RBF), ("TMH_SVC_LINEAR", hip.TMH_SVC_LINEAR),
                        ("TMH_FOREST_ROUTE_LDS", hip.TMH_FOREST_ROUTE_LDS),
                        ("TMH_FOREST_ROUTE_MEMORY", hip.TMH_FOREST_ROUTE_MEMORY)):
        assert "#define %s %d\n" % (name, value) in text, name
    from tmlibrary_amd.tools import supervised
    for name, value in (("TMH_FOREST_MAX_CLASSES", supervised.MAX_FOREST_CLASSES),
                        ("TMH_FOREST_MAX_TREES", supervised.MAX_FOREST_TREES),
                        ("TMH_SVC_MAX_CLASSES", supervised.MAX_SVC_CLASSES),
                        ("TMH_SVC_MAX_SV", supervised.MAX_SVC_VECTORS)):
        assert "#define %s %d\n" % (name, value) in text, name
    assert "#define TMH_FOREST_MAX_NODES (1 << 24)\n" in text


def create_forest(lib, m):
    from tmlibrary_amd import hip
    h = C.c_void_p()
    arrays = [np.ascontiguousarray(m[k], t) for k, t in (
        ("feature", np.int32), ("threshold", np.float64), ("left", np.int32), ("right", np.int32),
        ("leaf_row", np.int32), ("tree_root", np.int32), ("leaf_value", np.float64))]
    f, thr, le, ri, row, roots, value = arrays
    rc = lib.tmh_forest_create(hip.ptr(f), hip.ptr(thr), hip.ptr(le), hip.ptr(ri), hip.ptr(row),
                               f.size, hip.ptr(roots), roots.size, hip.ptr(value), value.shape[0],
                               value.shape[1], int(m["n_features"]), C.byref(h))
    return rc, h


def test_create_refuses_malformed_models_before_any_upload():
    """validation comes first, so the refusals need no device"""
    from tmlibrary_amd import hip
    lib = hip.load_library()
    for name, model in cases.malformed_forests().items():
        rc, h = create_forest(lib, model)
        assert rc == hip.TMH_EINVAL and not h.value, name
        assert lib.tmh_last_error(), name
    # the bounds are checked before any array is read: the small arrays stand in
    f = {k: np.ascontiguousarray(v) for k, v in cases.small_forest().items()}
    h = C.c_void_p()
    for nodes, text in ((1 << 24, b"2^24"), (0, b"2^24"), ((1 << 24) + 5, b"2^24")):
        rc = lib.tmh_forest_create(hip.ptr(f["feature"]), hip.ptr(f["threshold"]),
                                   hip.ptr(f["left"]), hip.ptr(f["right"]), hip.ptr(f["leaf_row"]),
                                   nodes, hip.ptr(f["tree_root"]), 2, hip.ptr(f["leaf_value"]), 5, 2,
                                   3, C.byref(h))
        assert rc == hip.TMH_EINVAL and text in lib.tmh_last_error() and not h.value, nodes
    rc, _ = create_forest(lib, cases.malformed_forests()["child_equals_parent"])
    assert b"greater than its parent" in lib.tmh_last_error()
    ok = cases.small_forest()
    for changes, text in ((dict(n_features=257), b"256 features"),
                          (dict(n_features=0), b"256 features"),
                          (dict(leaf_value=np.zeros((5, 65))), b"n_classes"),
                          (dict(leaf_value=np.zeros((5, 1))), b"n_classes"),
                          (dict(tree_root=np.zeros(257, np.int32)), b"n_trees")):
        rc, _ = create_forest(lib, dict(ok, **changes))
        assert rc == hip.TMH_EINVAL and text in lib.tmh_last_error(), text
    sv = cases.small_svc()
    h = C.c_void_p()

    def create_svc(**changes):
        m = dict(sv, **changes)
        a = [np.ascontiguousarray(m[k], t) for k, t in (("sv", np.float64), ("n_sv", np.int32),
                                                        ("coef", np.float64), ("rho", np.float64))]
        return lib.tmh_svc_create(int(m.get("code", 0)), float(m["gamma"]), hip.ptr(a[0]),
                                  a[0].shape[0], a[0].shape[1], hip.ptr(a[1]), a[1].size,
                                  hip.ptr(a[2]), hip.ptr(a[3]), C.byref(h))

    a = [np.ascontiguousarray(sv[k], t) for k, t in (("sv", np.float64), ("n_sv", np.int32),
                                                      ("coef", np.float64), ("rho", np.float64))]
    for m, d, k, text in ((65537, 2, 3, b"65,536"), (0, 2, 3, b"65,536"), (5, 257, 3, b"256 features"),
                          (5, 0, 3, b"256 features"), (5, 2, 1, b"2 .. 16"), (5, 2, 17, b"2 .. 16")):
        rc = lib.tmh_svc_create(0, 0.5, hip.ptr(a[0]), m, d, hip.ptr(a[1]), k, hip.ptr(a[2]),
                                hip.ptr(a[3]), C.byref(h))
        assert rc == hip.TMH_EINVAL and text in lib.tmh_last_error() and not h.value, (m, d, k)
    for changes, text in ((dict(code=2), b"rbf or linear"), (dict(gamma=0.0), b"gamma"),
                          (dict(gamma=np.nan), b"gamma"),
                          (dict(n_sv=np.array([2, 2, 2], np.int32)), b"add up"),
                          (dict(n_sv=np.array([6, -1, 0], np.int32)), b"negative"),
                          (dict(rho=np.array([0.1, np.inf, 0.0])), b"rho"),
                          (dict(n_sv=np.zeros(17, np.int32)), b"2 .. 16")):
        assert create_svc(**changes) == hip.TMH_EINVAL and text in lib.tmh_last_error(), text
    assert lib.tmh_forest_predict(None, None, 1, None, None) == hip.TMH_EINVAL
    assert lib.tmh_svc_predict(None, None, 1, None, None, None, None) == hip.TMH_EINVAL


# ---- the tool: payload handling ---------------------------------------------------------

def make_store(n=40):
    from tmlibrary_amd.tools.base import FeatureStore
    store = FeatureStore(seed=3)
    ids = np.arange(100, 100 + n)[::-1]
    values = np.stack([ids * 1.0, (ids % 7) * 2.0, ids * 3.0], axis=1)
    store.add_mapobject_type("Cells", ids, ["a", "b", "c"], values)
    return store


def payload(method="svm", **options):
    return {"chosen_object_type": "Cells", "selected_features": ["a", "b"],
            "training_classes": [{"name": "low", "object_ids": [100, 102, 104], "color": "#ff0000"},
                                 {"name": "high", "object_ids": [135, 137, 139], "color": "#00ff00"}],
            "options": dict({"method": method, "n_fold_cv": 2}, **options)}


class Recorder(object):
    """a model that labels on the host, so that the tool's plumbing is seen without a GPU"""

    def __init__(self):
        self.calls = []

    def predict(self, X, scaler=None):
        self.calls.append((X.shape, scaler))
        return np.where(X[:, 0] > 120.0, 1.0, 0.0)


def test_payload_handling():
    from tmlibrary_amd.tools import Classification, Clustering
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    store = make_store()
    tool = Classification(1, store=store)
    assert Classification.__options__ == {"method": ["randomforest", "svm"], "n_fold_cv": 10}
    assert Classification.n_test == 10 ** 6
    with pytest.raises(ValueError, match='Unknown method "logisticregression".'):
        tool.process_request(1, payload("logisticregression"))
    with pytest.raises(KeyError):
        tool.process_request(1, {k: v for k, v in payload().items() if k != "training_classes"})
    assert not store.results        # nothing was registered by a refused request
    with pytest.raises(NotSupportedError, match="Logistic regression"):
        tool.train_supervised(None, {}, "logisticregression", 3)
    # the base class's method stays unbuilt; the classification tool overrides it
    with pytest.raises(NotSupportedError, match="not built"):
        Clustering(1, store=store).train_supervised(None, {}, "svm", 3)
    assert Classification.train_supervised is not Clustering.train_supervised

    seen = {}
    recorder = Recorder()

    def fake_train(feature_data, labels, method, n_fold_cv, random_state=None):
        seen.update(index=list(feature_data.index), labels=dict(labels), method=method,
                    n_fold_cv=n_fold_cv, random_state=random_state, shape=feature_data.values.shape)
        return recorder, "the scaler"

    tool.train_supervised = fake_train
    tool.n_test = 16
    rid = tool.process_request(7, payload("randomforest", random_state=5))
    assert seen["index"] == [100, 102, 104, 135, 137, 139] and seen["shape"] == (6, 2)
    assert seen["labels"] == {100: 0.0, 102: 0.0, 104: 0.0, 135: 1.0, 137: 1.0, 139: 1.0}
    assert (seen["method"], seen["n_fold_cv"], seen["random_state"]) == ("randomforest", 2, 5)
    result = store.results[rid]
    assert result["type"] == "SupervisedClassifierToolResult" and result["submission_id"] == 7
    assert np.array_equal(result["attributes"]["unique_labels"], [0.0, 1.0])
    assert result["attributes"]["label_map"] == {0.0: {"name": "low", "color": "#ff0000"},
                                                 1.0: {"name": "high", "color": "#00ff00"}}
    assert [c[0] for c in recorder.calls] == [(16, 2), (16, 2), (8, 2)]     # batches of n_test
    assert all(c[1] == "the scaler" for c in recorder.calls)
    assert result["values"] == {i: int(i > 120) for i in range(100, 140)}


def test_training_without_scikit_learn_is_refused_by_name(monkeypatch):
    import builtins
    from tmlibrary_amd.tools import supervised
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    real = builtins.__import__

    def no_sklearn(name, *args, **kwargs):
        if name == "sklearn" or name.startswith("sklearn."):
            raise ImportError("No module named 'sklearn'")
        return real(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", no_sklearn)
    with pytest.raises(NotSupportedError, match="scikit-learn"):
        supervised.train_supervised(None, {}, "svm", 3)
