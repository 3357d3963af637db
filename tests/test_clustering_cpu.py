"""CPU: the clustering tool's rules and its Python layer.

The numpy literal (tests/clustering_literal.py) equals the recorded
scikit-learn results (tests/golden/clustering_*.npz) and, where scikit-learn
imports, scikit-learn itself; the rank / lerp / median arithmetic the host does
around the device's order statistics is bit-exact against numpy; the classes'
argument checks, the payload handling and the FeatureStore need no GPU.
"""
import functools
import os

import numpy as np
import pytest

import clustering_cases as cases
import clustering_literal as lit
from util import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, "clustering_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name):
    return cases.kmeans_case(name)


@functools.lru_cache(maxsize=None)
def literal_fit(name, tol):
    c = case(name)
    return lit.lloyd(c["Xs"], c["C0"], tol=tol)


def centre_bound(Xs):
    return Xs.shape[0] * lit.EPS * np.abs(Xs).max()


# ---- the literal against the goldens and scikit-learn -----------------------------

@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES) + list(cases.SCALER_ONLY_CASES))
def test_literal_scaler_equals_golden(name):
    X = cases.all_scaler_inputs()[name] if name in cases.SCALER_ONLY_CASES else case(name)["X"]
    center, scale = lit.robust_fit(X)
    g = golden(name)
    assert np.array_equal(center, g["center"]) and np.array_equal(scale, g["scale"])


@pytest.mark.parametrize("tol,prefix", [(0.0, "t0_"), (1e-4, "td_")])
@pytest.mark.parametrize("name", cases.GOLDEN_CASES)
def test_literal_lloyd_equals_golden(name, tol, prefix):
    labels, C, inertia, n_iter, tol_abs = literal_fit(name, tol)
    g = golden(name)
    Xs = case(name)["Xs"]
    assert np.array_equal(labels, g[prefix + "labels"])
    assert n_iter == int(g[prefix + "n_iter"])
    assert np.abs(C - g[prefix + "centres"]).max() <= centre_bound(Xs)
    assert abs(inertia - float(g[prefix + "inertia"])) <= Xs.shape[0] * lit.EPS * inertia
    assert tol_abs == float(g[prefix + "tol_abs"])


@pytest.mark.parametrize("name", ["n4097_d3_k2", "n5000_d7_k4_blobs", "one_empty"])
def test_literal_equals_sklearn(name):
    sk_cluster = pytest.importorskip("sklearn.cluster")
    sk_pre = pytest.importorskip("sklearn.preprocessing")
    c = case(name)
    sc = sk_pre.RobustScaler(quantile_range=(1.0, 99.0)).fit(c["X"])
    assert np.array_equal(sc.center_, c["center"]) and np.array_equal(sc.scale_, c["scale"])
    assert np.array_equal(sc.transform(c["X"]), c["Xs"])
    km = sk_cluster.KMeans(n_clusters=c["k"], init=c["C0"], n_init=1, algorithm="lloyd",
                           tol=0.0).fit(c["Xs"])
    labels, C, inertia, n_iter, _ = literal_fit(name, 0.0)
    assert np.array_equal(km.labels_, labels) and km.n_iter_ == n_iter
    assert np.abs(km.cluster_centers_ - C).max() <= centre_bound(c["Xs"])


def test_two_empty_case_is_what_it_says():
    c = case("two_empty")
    labels, mind, _ = lit.assign(c["Xs"], c["C0"])
    counts = np.bincount(labels, minlength=c["k"])
    assert list(np.flatnonzero(counts == 0)) == [1, 3]
    C1 = lit.update(c["Xs"], labels, mind, c["C0"])
    order = np.lexsort((np.arange(mind.size), -mind))
    assert np.array_equal(C1[1], c["Xs"][order[0]]) and np.array_equal(C1[3], c["Xs"][order[1]])


def test_seeding_literal_follows_sklearn_rule():
    c = case("n5000_d7_k4_blobs")
    first, draws = lit.seed_draws(np.random.RandomState(5), c["Xs"].shape[0], 4)
    assert draws.shape == (3, lit.n_local_trials(4)) == (3, 3)
    indices, trace = lit.kmeans_plusplus(c["Xs"], 4, first, draws)
    assert indices[0] == first and len(set(indices.tolist())) == 4
    for step in trace:
        for t, row in zip(step["targets"], step["cand"]):
            assert step["cumsum"][row] >= t and (row == 0 or step["cumsum"][row - 1] < t)
        assert step["best"] == int(np.argmin(step["pots"]))


# ---- rank, lerp, median: the host's arithmetic around the order statistics --------------

@pytest.mark.parametrize("name", list(cases.KMEANS_CASES) + list(cases.SCALER_ONLY_CASES))
def test_host_finish_is_bit_exact_against_numpy(name):
    from tmlibrary_amd.tools.base import RobustScaler
    X = cases.all_scaler_inputs()[name]
    d = X.shape[1]
    values, gammas = np.empty((d, 6)), np.empty((d, 2))
    for f in range(d):
        col = np.sort(X[:, f][~np.isnan(X[:, f])])
        ranks, gammas[f] = RobustScaler.column_ranks(col.size, (1.0, 99.0))
        assert ranks == lit.column_ranks(col.size)[0]
        values[f] = col[ranks]
    center, scale = RobustScaler.finish(values, gammas)
    assert np.array_equal(center, np.nanmedian(X, axis=0))
    spread = np.nanpercentile(X, 99.0, axis=0) - np.nanpercentile(X, 1.0, axis=0)
    assert np.array_equal(scale, np.where(spread == 0.0, 1.0, spread))
    lc, ls = lit.robust_fit(X)
    assert np.array_equal(center, lc) and np.array_equal(scale, ls)


def test_median_is_not_the_percentile_lerp():
    # a pair for which (a + b) / 2 and the 50 % lerp b - (b - a) * 0.5 differ in the last bit
    from tmlibrary_amd.tools.base import RobustScaler
    a, b = np.float64(-0.977277879876411), np.float64(1.8675579901499675)
    half = lit.lerp(a, b, 0.5)
    assert half == np.percentile([a, b], 50.0) and half != (a + b) / 2
    x = np.array([[a], [b]])
    assert np.nanmedian(x) == (a + b) / 2
    assert lit.robust_fit(x)[0][0] == (a + b) / 2
    ranks, gammas = RobustScaler.column_ranks(2, (1.0, 99.0))
    center, _ = RobustScaler.finish(np.array([[a, b][r] for r in ranks])[None], gammas[None])
    assert center[0] == (a + b) / 2 and center[0] != half


def test_zero_scale_becomes_one():
    g = golden("n3001_d33_k9")
    assert g["scale"][5] == 1.0 and g["center"][5] == 3.25


# ---- the classes' argument checks -------------------------------------------------------------

def test_limits_are_refused_by_name():
    from tmlibrary_amd.tools import base
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    with pytest.raises(NotSupportedError, match="256"):
        base.check_limits(10, 257)
    with pytest.raises(NotSupportedError, match="64"):
        base.check_limits(100, 4, 65)
    with pytest.raises(NotSupportedError, match="8192"):
        base.check_limits(100, 256, 33)
    with pytest.raises(NotSupportedError, match="2\\*\\*31"):
        base.check_limits(2 ** 31, 4)
    base.check_limits(2 ** 31 - 1, 256, 32)
    with pytest.raises(NotSupportedError, match="8192"):
        base.KMeans(n_clusters=33).fit(np.zeros((100, 256)))


def test_kmeans_argument_checks_need_no_gpu():
    from tmlibrary_amd.tools.base import KMeans, RobustScaler
    X = np.arange(12.0).reshape(6, 2)
    with pytest.raises(ValueError, match="n_samples=6 should be >= n_clusters=7"):
        KMeans(n_clusters=7).fit(X)
    with pytest.raises(ValueError, match="n_clusters"):
        KMeans(n_clusters=0).fit(X)
    with pytest.raises(ValueError, match="shape of the initial centers"):
        KMeans(n_clusters=2, init=np.zeros((2, 3))).fit(X)
    with pytest.raises(ValueError, match="init must be"):
        KMeans(n_clusters=2, init="random").fit(X)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        KMeans(n_clusters=2, init=X[:2]).fit(bad)
    with pytest.raises(ValueError, match="2D"):
        KMeans(n_clusters=2).fit(np.arange(4.0))
    with pytest.raises(ValueError, match="not fitted"):
        KMeans(n_clusters=2).predict(X)
    with pytest.raises(ValueError, match="Invalid quantile range"):
        RobustScaler(quantile_range=(60.0, 40.0))
    with pytest.raises(ValueError, match="not fitted"):
        RobustScaler().transform(X)


def test_draws_follow_the_call_order():
    from tmlibrary_amd.tools.base import KMeans
    assert [KMeans.n_local_trials(k) for k in (1, 2, 8, 20, 64)] == [2, 2, 4, 4, 6]
    rs = np.random.RandomState(7)
    first, draws = lit.seed_draws(np.random.RandomState(7), 1000, 8)
    assert first == rs.randint(1000)
    assert np.array_equal(draws[0], rs.uniform(size=4))


# ---- the tool: payload handling and the FeatureStore ------------------------------------------

def make_store(n=10, seed=3):
    from tmlibrary_amd.tools.base import FeatureStore
    store = FeatureStore(seed=seed)
    ids = np.arange(100, 100 + n)[::-1]            # stored in any order
    values = np.stack([ids * 1.0, ids * 2.0, ids * 3.0], axis=1)
    store.add_mapobject_type("Cells", ids, ["a", "b", "c"], values)
    return store


def test_feature_store_batching():
    store = make_store()
    batches = store.partition_mapobjects("Cells", 4)
    assert [len(b) for b in batches] == [4, 4, 2]
    assert np.array_equal(np.concatenate(batches), np.arange(100, 110))
    subset = store.get_random_mapobject_subset("Cells", 6)
    assert len(subset) == 6 == len(set(subset.tolist())) and set(subset) <= set(range(100, 110))
    assert sorted(store.get_random_mapobject_subset("Cells", 10 ** 6).tolist()) == list(range(100, 110))
    t = store.load_feature_values("Cells", ["c", "a"], np.array([105, 101]))
    assert np.array_equal(t.values, [[315.0, 105.0], [303.0, 101.0]])
    assert np.array_equal(t.index, [105, 101]) and t.columns == ["c", "a"]
    assert np.array_equal(np.asarray(t), t.values)
    with pytest.raises(ValueError, match='Unknown feature "z"'):
        store.load_feature_values("Cells", ["z"])
    with pytest.raises(ValueError, match="Unknown mapobject id"):
        store.load_feature_values("Cells", ["a"], [99])
    with pytest.raises(ValueError, match='Unknown mapobject type "Nuclei"'):
        store.partition_mapobjects("Nuclei", 4)
    rid = store.register_result(1, "Cells", result_type="ScalarToolResult", unique_labels=[0, 1])
    assert store.register_result(1, "Cells", result_type="ScalarToolResult") == rid
    assert store.register_result(2, "Cells", result_type="ScalarToolResult") != rid


def test_payload_handling():
    from tmlibrary_amd.tools import Clustering, FeatureStore
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    store = make_store()
    with pytest.raises(ValueError, match="FeatureStore is required"):
        Clustering(1)
    with pytest.raises(TypeError):
        Clustering(1, store=object())
    tool = Clustering(1, store=store)
    assert Clustering.n_train == Clustering.n_test == 10 ** 6
    payload = {"chosen_object_type": "Cells", "selected_features": ["a", "b"],
               "options": {"k": 2, "method": "spectral"}}
    with pytest.raises(ValueError, match='Unknown method "spectral".'):
        tool.process_request(1, payload)
    with pytest.raises(ValueError, match='Unknown method "spectral".'):
        tool.train_unsupervised(np.zeros((4, 2)), 2, "spectral")
    with pytest.raises(KeyError):
        tool.process_request(1, {"selected_features": [], "options": {"k": 2, "method": "kmeans"}})
    with pytest.raises(NotSupportedError):
        tool.train_supervised(None, {}, "svm", 3)
    assert not store.results        # nothing was registered by a refused request
    assert isinstance(store, FeatureStore)


def test_abi_agreement_covers_the_new_symbols():
    from tmlibrary_amd import hip
    text = open(os.path.join(REPO, "include", "tmhip.h")).read()
    lib = hip.load_library()
    for stem in ("column_census", "column_select", "robust_scale", "kmeans_seed", "kmeans_predict",
                 "kmeans_fit"):
        for name in ("tmh_" + stem, "tmh_" + stem + "_device"):
            assert name in hip.SIGNATURES and name + "(" in text and hasattr(lib, name)
    assert hip.ABI_VERSION == 9 == lib.tmh_abi_version()
