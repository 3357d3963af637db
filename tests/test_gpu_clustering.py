"""GPU: the clustering tool against the recorded
scikit-learn results and the numpy literal.

Comparison rules.  A row is *close* for a set of centres when its two smallest
squared distances differ by less than 64 d 2^-52 of their sum -- the rounding
bound of a d-term sum with FMA contraction, with margin; label comparisons may
leave out close rows, up to 0.1 % of n (the golden generator asserts that the
literal meets none at any iteration, so the allowance is a condition, not a
tolerance).  Centres and inertia are compared with the bound of reordering an
n-term sum, n 2^-52 max|X_scaled| (inertia: n 2^-52 inertia); iteration counts
exactly; tol_abs to 1e-12 relative; the scaler bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import clustering_cases as cases
import clustering_literal as lit
from test_clustering_cpu import case, centre_bound, golden, literal_fit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


def scaler_of(c):
    from tmlibrary_amd.tools.base import RobustScaler
    s = RobustScaler()
    s.center_, s.scale_, s.n_features_in_ = c["center"], c["scale"], c["X"].shape[1]
    return s


def assert_labels(got, want, Xs, centres):
    """equal outside the rows close for `centres`, of which there may be 0.1 % of n"""
    _, _, D = lit.assign(Xs, centres)
    close = lit.close_rows(D, Xs.shape[1])
    assert close.sum() <= Xs.shape[0] // 1000
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)) & ~close)
    assert bad.size == 0, "%d labels differ, first at row %d" % (bad.size, bad[0])


# ---- census and select ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n3001_d33_k9", "nan_column", "n1000_d256_k32"])
def test_census_counts_and_moments(L, name):
    from tmlibrary_amd import hip
    X = cases.all_scaler_inputs()[name].copy()
    X[7, 0] = np.inf
    X[9, X.shape[1] - 1] = -np.inf
    n, d = X.shape
    count, n_inf = np.zeros(d, np.int64), np.zeros(d, np.int64)
    hip.check(L.tmh_column_census(hip.ptr(X), n, d, None, None, hip.ptr(count), hip.ptr(n_inf),
                                  None, None))
    assert np.array_equal(count, (~np.isnan(X)).sum(axis=0))
    assert np.array_equal(n_inf, np.isinf(X).sum(axis=0))
    X = cases.all_scaler_inputs()[name]
    center, scale = lit.robust_fit(X)
    mean, var = np.zeros(d), np.zeros(d)
    hip.check(L.tmh_column_census(hip.ptr(X), n, d, hip.ptr(center), hip.ptr(scale),
                                  hip.ptr(count), hip.ptr(n_inf), hip.ptr(mean), hip.ptr(var)))
    Xs = lit.robust_transform(X, center, scale)
    w_mean, w_var = np.nanmean(Xs, axis=0), np.nanvar(Xs, axis=0)
    assert np.abs(mean - w_mean).max() <= n * lit.EPS * np.nanmax(np.abs(Xs))
    assert np.allclose(var, w_var, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", ["n4097_d3_k2", "nan_column", "zeros_and_duplicates",
                                  "n1000_d256_k32"])
def test_select_returns_the_sorted_value(L, name):
    from tmlibrary_amd import hip
    X = cases.all_scaler_inputs()[name]
    n, d = X.shape
    r = 7
    ranks = np.zeros((d, r), dtype=np.int64)
    want = np.zeros((d, r))
    for f in range(d):
        col = np.sort(X[:, f][~np.isnan(X[:, f])])
        m = col.size
        ranks[f] = [0, 1, m // 100, (m - 1) // 2, m // 2, m - 2, m - 1]
        want[f] = col[ranks[f]]
    got = np.full((d, r), np.nan)
    hip.check(L.tmh_column_select(hip.ptr(X), n, d, None, hip.ptr(ranks), r, hip.ptr(got)))
    assert (got == want).all()      # by value: -0.0 == +0.0
    # with the census' counts handed in (no second census): the same values
    count = np.ascontiguousarray((~np.isnan(X)).sum(axis=0), dtype=np.int64)
    again = np.full((d, r), np.nan)
    hip.check(L.tmh_column_select(hip.ptr(X), n, d, hip.ptr(count), hip.ptr(ranks), r,
                                  hip.ptr(again)))
    assert again.tobytes() == got.tobytes()
    ranks[0, 0] = count[0]          # one past the column's last rank
    assert L.tmh_column_select(hip.ptr(X), n, d, hip.ptr(count), hip.ptr(ranks), r,
                               hip.ptr(again)) == hip.TMH_EINVAL


@pytest.mark.parametrize("name", list(cases.GOLDEN_CASES) + list(cases.SCALER_ONLY_CASES))
def test_scaler_fit_is_bit_exact(L, name):
    from tmlibrary_amd.tools.base import RobustScaler
    X = cases.all_scaler_inputs()[name]
    s = RobustScaler(quantile_range=(1.0, 99.0)).fit(X)
    g = golden(name)
    assert np.array_equal(s.center_, g["center"])
    assert np.array_equal(s.scale_, g["scale"])


# ---- transform ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n3001_d33_k9", "nan_column", "tile_above"])
def test_transform_is_bit_exact(L, name):
    from tmlibrary_amd.tools.base import RobustScaler
    X = cases.all_scaler_inputs()[name]
    s = RobustScaler().fit(X)
    got = s.transform(X)
    want = (X - s.center_) / s.scale_
    ok = ~np.isnan(X)
    assert np.array_equal(np.isnan(got), ~ok)
    assert got[ok].tobytes() == want[ok].tobytes()     # bits: the sign of zero included


@pytest.mark.parametrize("name", ["n3001_d33_k9", "tile_below", "one_empty"])
def test_scaling_on_load_gives_the_same_bytes(L, name):
    from tmlibrary_amd.tools.base import KMeans
    c = case(name)
    a = KMeans(n_clusters=c["k"], init=c["C0"]).fit(c["X"], scaler=scaler_of(c))
    b = KMeans(n_clusters=c["k"], init=c["C0"]).fit(c["Xs"])
    assert a.labels_.tobytes() == b.labels_.tobytes()
    assert a.cluster_centers_.tobytes() == b.cluster_centers_.tobytes()
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_ and a.tol_abs_ == b.tol_abs_
    assert a.predict(c["X"], scaler=scaler_of(c)).tobytes() == b.predict(c["Xs"]).tobytes()


# ---- predict ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.GOLDEN_CASES)
def test_predict_equals_literal(L, name):
    from tmlibrary_amd import hip
    c = case(name)
    centres = np.ascontiguousarray(golden(name)["t0_centres"])
    X = c["X"]
    n, d = X.shape
    labels = np.full(n, -1, dtype=np.int32)
    mind = np.zeros(n)
    hip.check(L.tmh_kmeans_predict(hip.ptr(X), n, d, c["k"], hip.ptr(c["center"]),
                                   hip.ptr(c["scale"]), hip.ptr(centres), hip.ptr(labels),
                                   hip.ptr(mind)))
    want, w_mind, _ = lit.assign(c["Xs"], centres)
    assert_labels(labels, want, c["Xs"], centres)
    assert np.allclose(mind, w_mind, rtol=64 * d * lit.EPS, atol=0.0)


def test_predict_labels_fewer_rows_than_clusters(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import KMeans
    c = case("n3001_d33_k9")
    centres = np.ascontiguousarray(golden("n3001_d33_k9")["t0_centres"])
    want, _, _ = lit.assign(c["Xs"], centres)
    model = KMeans(n_clusters=9)
    model.cluster_centers_ = centres
    for rows in (1, 5, 8):                      # all below k = 9
        got = model.predict(c["X"][:rows], scaler=scaler_of(c))
        assert got.dtype == np.int32 and np.array_equal(got, want[:rows])
    X = np.ascontiguousarray(c["Xs"][:3])
    labels = np.full(3, -1, np.int32)
    hip.check(L.tmh_kmeans_predict(hip.ptr(X), 3, 33, 9, None, None, hip.ptr(centres),
                                   hip.ptr(labels), None))
    assert np.array_equal(labels, want[:3])


# ---- fit from given centres ------------------------------------------------------------------

@pytest.mark.parametrize("tol,prefix", [(0.0, "t0_"), (1e-4, "td_")])
@pytest.mark.parametrize("name", cases.GOLDEN_CASES)
def test_fit_equals_golden(L, name, tol, prefix):
    from tmlibrary_amd.tools.base import KMeans
    c, g = case(name), golden(name)
    m = KMeans(n_clusters=c["k"], init=c["C0"], n_init=1, tol=tol).fit(c["X"], scaler=scaler_of(c))
    Xs = c["Xs"]
    n = Xs.shape[0]
    print("%s tol=%g: n_iter %d (golden %d), max centre diff %.3g (bound %.3g), inertia %.17g "
          "(golden %.17g)" % (name, tol, m.n_iter_, int(g[prefix + "n_iter"]),
                              np.abs(m.cluster_centers_ - g[prefix + "centres"]).max(),
                              centre_bound(Xs), m.inertia_, float(g[prefix + "inertia"])))
    assert m.n_iter_ == int(g[prefix + "n_iter"])
    assert_labels(m.labels_, g[prefix + "labels"], Xs, g[prefix + "centres"])
    assert np.abs(m.cluster_centers_ - g[prefix + "centres"]).max() <= centre_bound(Xs)
    assert abs(m.inertia_ - float(g[prefix + "inertia"])) <= n * lit.EPS * float(g[prefix + "inertia"])
    assert abs(m.tol_abs_ - float(g[prefix + "tol_abs"])) <= 1e-12 * float(g[prefix + "tol_abs"])


@pytest.mark.parametrize("tol", [0.0, 1e-4])
def test_two_empty_clusters_equal_literal(L, tol):
    from tmlibrary_amd.tools.base import KMeans
    c = case("two_empty")
    labels, centres, inertia, n_iter, tol_abs = literal_fit("two_empty", tol)
    m = KMeans(n_clusters=c["k"], init=c["C0"], tol=tol).fit(c["X"], scaler=scaler_of(c))
    assert m.n_iter_ == n_iter
    assert_labels(m.labels_, labels, c["Xs"], centres)
    assert np.abs(m.cluster_centers_ - centres).max() <= centre_bound(c["Xs"])
    assert abs(m.inertia_ - inertia) <= c["Xs"].shape[0] * lit.EPS * inertia
    # the first iteration alone: the two farthest rows became centres 1 and 3
    one = KMeans(n_clusters=c["k"], init=c["C0"], max_iter=1, tol=0.0).fit(c["Xs"])
    l0, mind, _ = lit.assign(c["Xs"], c["C0"])
    want = lit.update(c["Xs"], l0, mind, c["C0"])
    assert np.array_equal(one.cluster_centers_[[1, 3]], want[[1, 3]])
    assert np.abs(one.cluster_centers_ - want).max() <= centre_bound(c["Xs"])


@pytest.mark.parametrize("name", ["n2048_d128_k64", "n5000_d7_k4_blobs"])
def test_fit_is_reproducible(L, name):
    from tmlibrary_amd.tools.base import KMeans
    c = case(name)
    runs = [KMeans(n_clusters=c["k"], init=c["C0"]).fit(c["Xs"]) for _ in range(2)]
    assert runs[0].labels_.tobytes() == runs[1].labels_.tobytes()
    assert runs[0].cluster_centers_.tobytes() == runs[1].cluster_centers_.tobytes()
    assert runs[0].inertia_ == runs[1].inertia_ and runs[0].n_iter_ == runs[1].n_iter_


# ---- seeding -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,seed", [("n5000_d7_k4_blobs", 5), ("n3001_d33_k9", 6),
                                       ("tile_above", 7), ("n2048_d128_k64", 8)])
def test_seeding_follows_the_draws(L, name, seed):
    from tmlibrary_amd.tools.base import DeviceTable, KMeans
    c = case(name)
    Xs, k = c["Xs"], c["k"]
    n = Xs.shape[0]
    assert np.unique(Xs, axis=0).shape[0] == n
    first, draws = lit.seed_draws(np.random.RandomState(seed), n, k)
    trials = draws.shape[1]
    assert trials == KMeans.n_local_trials(k)
    with DeviceTable(c["X"], scaler_of(c)) as t:
        indices, centres, trace = KMeans.seed(t, k, first, draws, trace=True)
        again = KMeans.seed(t, k, first, draws)
    assert np.array_equal(indices, again[0]) and centres.tobytes() == again[1].tobytes()
    assert indices[0] == first and len(set(indices.tolist())) == k
    assert np.array_equal(centres, Xs[indices])
    # the literal's state follows the device's kept rows, so one row picked
    # within the tolerance does not carry into the later steps
    diff = Xs - Xs[first]
    closest = (diff * diff).sum(axis=1)
    for step in range(1, k):
        tr = trace[step - 1]
        targets, cand = tr[:trials], tr[trials:2 * trials].astype(np.int64)
        pots, kept = tr[2 * trials:3 * trials], int(tr[3 * trials])
        pot = closest.sum()
        slack = n * lit.EPS * pot
        assert np.abs(targets - draws[step - 1] * pot).max() <= slack
        cum = np.cumsum(closest)
        trial = np.empty((trials, n))
        for q in range(trials):
            i = cand[q]
            assert 0 <= i < n
            below = cum[i - 1] if i > 0 else 0.0
            assert below - slack <= targets[q] <= cum[i] + slack or \
                (i == n - 1 and targets[q] >= cum[i] - slack)
            diff = Xs - Xs[i]
            trial[q] = np.minimum(closest, (diff * diff).sum(axis=1))
        w_pots = trial.sum(axis=1)
        assert np.abs(pots - w_pots).max() <= n * lit.EPS * pot
        assert kept == int(np.argmin(w_pots))
        assert indices[step] == cand[kept]
        closest = trial[kept]


def test_one_cluster_from_kmeans_plusplus(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import KMeans
    c = case("n257_d1_k1")
    Xs = c["Xs"]
    n = Xs.shape[0]
    m = KMeans(n_clusters=1, random_state=4).fit(Xs)        # the default init
    assert np.array_equal(m.labels_, np.zeros(n, np.int32))
    assert abs(m.cluster_centers_[0, 0] - Xs.mean()) <= centre_bound(Xs)
    g = golden("n257_d1_k1")
    assert abs(m.inertia_ - float(g["td_inertia"])) <= n * lit.EPS * float(g["td_inertia"])
    # the C call itself: one centre is the first row, no draws, no trace
    idx, centre = np.full(1, -1, np.int32), np.zeros((1, 1))
    hip.check(L.tmh_kmeans_seed(hip.ptr(Xs), n, 1, 1, None, None, 41, None, 1, hip.ptr(idx),
                                hip.ptr(centre), None))
    assert idx[0] == 41 and centre[0, 0] == Xs[41, 0]
    wide = case("n5000_d7_k4_blobs")["Xs"]
    one = KMeans(n_clusters=1, random_state=0).fit(wide)
    assert np.abs(one.cluster_centers_[0] - wide.mean(axis=0)).max() <= centre_bound(wide)


def test_kmeans_plusplus_fit_end_to_end(L):
    from tmlibrary_amd.tools.base import KMeans
    c = case("n5000_d7_k4_blobs")
    a = KMeans(n_clusters=4, random_state=3, n_init=2).fit(c["Xs"])
    b = KMeans(n_clusters=4, random_state=3, n_init=2).fit(c["Xs"])
    assert a.labels_.tobytes() == b.labels_.tobytes() and a.inertia_ == b.inertia_
    single = KMeans(n_clusters=4, random_state=3, n_init=1).fit(c["Xs"])
    assert a.inertia_ <= single.inertia_
    labels, mind, _ = lit.assign(c["Xs"], a.cluster_centers_)
    assert_labels(a.labels_, labels, c["Xs"], a.cluster_centers_)
    assert abs(a.inertia_ - mind.sum()) <= (5000 + 64 * 7) * lit.EPS * mind.sum()


# ---- refusals ----------------------------------------------------------------------------------

def launches(L, name):
    ms, cnt = C.c_double(0.0), C.c_int64(0)
    assert L.tmh_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0
    return cnt.value


def test_refusals_launch_no_kmeans_kernel(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.tools.base import KMeans
    from tmlibrary_amd.workflow.align.api import NotSupportedError
    hip.check(L.tmh_profile_enable(1))
    hip.check(L.tmh_profile_reset())
    try:
        X = np.random.RandomState(1).normal(size=(300, 4))
        C0 = np.ascontiguousarray(X[:3])
        bad = X.copy()
        bad[17, 2] = np.nan
        worse = X.copy()
        worse[5, 0] = np.inf
        out_c, labels = np.zeros((3, 4)), np.zeros(300, np.int32)
        inertia, tol_abs, n_iter = C.c_double(), C.c_double(), C.c_int()

        def fit(x, n, d, k, c0):
            return L.tmh_kmeans_fit(hip.ptr(x), n, d, k, None, None, hip.ptr(c0), 10, 1e-4,
                                    hip.ptr(out_c), hip.ptr(labels), C.byref(inertia),
                                    C.byref(n_iter), C.byref(tol_abs))

        for x in (bad, worse):
            assert fit(x, 300, 4, 3, C0) == hip.TMH_EINVAL
            assert b"NaN or infinite" in L.tmh_last_error()
            assert L.tmh_kmeans_predict(hip.ptr(x), 300, 4, 3, None, None, hip.ptr(C0),
                                        hip.ptr(labels), None) == hip.TMH_EINVAL
            assert b"NaN or infinite" in L.tmh_last_error()
        draws = np.full((2, 3), 0.5)
        idx = np.zeros(3, np.int32)
        assert L.tmh_kmeans_seed(hip.ptr(bad), 300, 4, 3, None, None, 0, hip.ptr(draws), 3,
                                 hip.ptr(idx), hip.ptr(out_c), None) == hip.TMH_EINVAL
        # k * d over the limit, d and k over theirs, k > n
        wide = np.zeros((100, 256))
        c_wide = np.zeros((33, 256))
        assert fit(wide, 100, 256, 33, c_wide) == hip.TMH_EINVAL
        assert b"8,192" in L.tmh_last_error()
        assert fit(wide, 100, 257, 2, c_wide) == hip.TMH_EINVAL and b"256" in L.tmh_last_error()
        assert fit(wide, 6400, 4, 65, c_wide) == hip.TMH_EINVAL and b"64" in L.tmh_last_error()
        assert fit(X, 2, 4, 3, C0) == hip.TMH_EINVAL
        assert b"more clusters than rows" in L.tmh_last_error()
        # the Python layer names the limit before anything is uploaded
        with pytest.raises(NotSupportedError, match="8192"):
            KMeans(n_clusters=33, init=c_wide).fit(wide)
        with pytest.raises(ValueError, match="NaN"):
            KMeans(n_clusters=3, init=C0).fit(bad)
        for kernel in ("kmeans_assign", "kmeans_update", "kmeans_seed"):
            assert launches(L, kernel) == 0, kernel
        good = KMeans(n_clusters=3, init=C0, max_iter=1).fit(X)
        assert launches(L, "kmeans_assign") > 0      # the counter does count
        hip.check(L.tmh_profile_reset())
        with pytest.raises(ValueError, match="NaN"):
            good.predict(bad)
        # overlapping buffers (device forms)
        with hip.DeviceBuffer.from_array(X) as dev:
            inside = dev.at(64)
            assert L.tmh_kmeans_fit_device(dev, 300, 4, 3, None, None, hip.ptr(C0), 10, 1e-4,
                                           hip.ptr(out_c), inside, C.byref(inertia),
                                           C.byref(n_iter), C.byref(tol_abs),
                                           None) == hip.TMH_EINVAL
            assert b"overlap" in L.tmh_last_error()
            assert L.tmh_kmeans_predict_device(dev, 300, 4, 3, None, None, hip.ptr(C0), inside,
                                               None, None) == hip.TMH_EINVAL
            assert b"overlap" in L.tmh_last_error()
            cs = np.ones(4)
            assert L.tmh_robust_scale(hip.ptr(X), 300, 4, hip.ptr(cs), hip.ptr(cs),
                                      hip.ptr(X)) == hip.TMH_OK   # host form: staged, no aliasing
            with hip.DeviceBuffer.from_array(cs) as dcs:
                assert L.tmh_robust_scale_device(dev, 300, 4, dcs, dcs, inside,
                                                 None) == hip.TMH_EINVAL
                assert b"overlap" in L.tmh_last_error()
        for kernel in ("kmeans_assign", "kmeans_update", "kmeans_seed"):
            assert launches(L, kernel) == 0, kernel
    finally:
        hip.check(L.tmh_profile_enable(0))


# ---- end to end ---------------------------------------------------------------------------------

def test_process_request_labels_two_groups(L):
    from tmlibrary_amd.tools import Clustering, FeatureStore
    rs = np.random.RandomState(41)
    n = 20000
    group = rs.randint(2, size=n)
    values = rs.normal(size=(n, 4)) + np.where(group[:, None] == 1, 25.0, -25.0)
    values[:, 3] = rs.normal(size=n)                   # a feature the tool does not select
    ids = rs.permutation(np.arange(1000, 1000 + n))
    store = FeatureStore(seed=2)
    store.add_mapobject_type("Cells", ids, ["f0", "f1", "f2", "noise"], values)

    class SmallBatches(Clustering):
        n_test = 2857        # eight batches, the last of one object: fewer than k

    tool = SmallBatches(1, store=store)
    rid = tool.process_request(9, {"chosen_object_type": "Cells",
                                   "selected_features": ["f0", "f1", "f2"],
                                   "options": {"k": 2, "method": "kmeans"}})
    result = store.results[rid]
    assert result["type"] == "ScalarToolResult" and result["submission_id"] == 9
    assert list(result["attributes"]["unique_labels"]) == [0, 1]
    got = np.array([result["values"][int(i)] for i in ids])
    assert len(result["values"]) == n
    assert np.array_equal(got, group) or np.array_equal(got, 1 - group)
    # predict hands back a Series when the input had an index
    batch = store.load_feature_values("Cells", ["f0", "f1", "f2"], ids[:5])
    model, scaler = tool.train_unsupervised(batch.values.repeat(3, axis=0), 2, "kmeans")
    series = tool.predict(batch, model, scaler)
    assert list(series.index) == list(batch.index) and len(series) == 5
