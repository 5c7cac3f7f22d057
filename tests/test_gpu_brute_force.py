"""The exact brute-force searcher (smx_bf_*, scann_amd/csrc/smx_brute_force.hip)
against the oracle.

Batched reference: oracle.partition_topl(q, db, metric, k) with the database
as "centers" -- the reference's DenseDistanceManyToManyTopK, exact top-k by
(score, row id); ids and distance bits must be equal.  Single-query
reference: oracle.exact_distance per row (DenseDistanceOneToMany), ordered
by (distance, id)."""
import numpy as np
import pytest

from scann_amd import _native, scann_ops_pybind, synthetic
from scann_amd.brute_force import BruteForceIndex

pytestmark = pytest.mark.gpu

DOT, L2 = 0, 1


def _data(n, dim, nq, seed, metric):
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    if metric == DOT and dim > 1:
        db /= np.linalg.norm(db, axis=1, keepdims=True)
    return db, q


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_batched(oracle, db, q, metric, k, got):
    """(idx, dist, count) of a batched search == the oracle's top-k."""
    idx, dist, cnt = got
    n = db.shape[0]
    m = min(k, n)
    oi, od = oracle.partition_topl(q, db, metric, m)
    assert np.all(cnt == m)
    np.testing.assert_array_equal(idx[:, :m], oi.astype(np.uint32))
    np.testing.assert_array_equal(_bits(dist[:, :m]), _bits(od))
    # padding: id 0 / NaN
    assert np.all(idx[:, m:] == 0) and np.all(np.isnan(dist[:, m:]))


def _handle(db, metric):
    return _native.NativeBruteForce(BruteForceIndex(db, metric), device=0)


# dims 1 / 3 (odd: the (-0)(+0) padding), 100 / 128 (one staging round), 130 /
# 257 (the chunked path); rows 1 .. 4097 (partial tiles, several blocks);
# nq 1 .. 130 (partial query tiles); k 1 .. 256; k > N at N = 5
SHAPES = [
    # dim, N, nq, k
    (1, 1, 1, 1),
    (1, 65, 33, 10),
    (3, 31, 33, 10),
    (3, 4097, 65, 256),
    (100, 64, 65, 10),
    (100, 4097, 130, 100),
    (128, 65, 130, 100),
    (128, 1000, 1, 1),
    (130, 1000, 33, 256),
    (257, 4097, 65, 10),
    (100, 5, 33, 10),
]


@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim,n,nq,k", SHAPES)
def test_shapes(oracle, dim, n, nq, k, metric):
    db, q = _data(n, dim, nq, 1000 * dim + n + metric, metric)
    h = _handle(db, metric)
    try:
        _check_batched(oracle, db, q, metric, k, h.search_batched(q, k))
    finally:
        h.close()


@pytest.fixture(scope="module")
def mid():
    """N = 20000, dim 100, nq 100 (dot, unit rows)."""
    return _data(20000, 100, 100, 77, DOT)


@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("k", [10, 100])
def test_many_passes(oracle, mid, k, metric):
    """first_pass_rows = 128: passes of 128, 512, 2048, 8192 and a partial
    9120 rows."""
    db, q = mid
    h = _handle(db, metric)
    try:
        h.set_tuning(128, 0)
        got = h.search_batched(q, k)
        st = h.stats()
        print("stats", st)
        assert st["passes"] >= 5
        _check_batched(oracle, db, q, metric, k, got)
    finally:
        h.close()


@pytest.fixture(scope="module")
def adversarial():
    """Every query the unit vector e; rows (i / N) e + 1e-3 noise: each later
    row beats (almost all) earlier ones under -dot."""
    n, dim, nq = 20000, 100, 100
    rng = np.random.default_rng(9)
    e = np.zeros(dim, np.float32)
    e[7] = 1.0
    db = (np.arange(n, dtype=np.float32)[:, None] / np.float32(n)) * e[None, :]
    db = (db + np.float32(1e-3) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    q = np.repeat(e[None, :], nq, axis=0)
    return db, q


@pytest.mark.parametrize("reverse", [False, True])
def test_adversarial_order(oracle, adversarial, reverse):
    db, q = adversarial
    if reverse:
        db = np.ascontiguousarray(db[::-1])
    h = _handle(db, DOT)
    try:
        # 64 candidates against passes of 256, 1024, ... rows that all survive
        h.set_tuning(0, 64)
        got = h.search_batched(q, 10)
        st = h.stats()
        print("stats", st)
        if not reverse:
            assert st["fallback_pieces"] > 0
            assert st["max_candidates"] > 64
        _check_batched(oracle, db, q, DOT, 10, got)
    finally:
        h.close()


@pytest.mark.parametrize("metric", [DOT, L2])
def test_identical_rows(metric):
    rng = np.random.default_rng(3)
    row = rng.standard_normal(100).astype(np.float32)
    db = np.repeat(row[None, :], 300, axis=0)
    q = rng.standard_normal((33, 100)).astype(np.float32)
    h = _handle(db, metric)
    try:
        idx, dist, cnt = h.search_batched(q, 10)
        np.testing.assert_array_equal(idx, np.tile(np.arange(10, dtype=np.uint32), (33, 1)))
        assert np.all(cnt == 10)
        assert np.all(_bits(dist) == _bits(dist[:, :1]))
        # every row ties at the threshold: with a buffer below N they overflow it
        h.set_tuning(0, 64)
        idx2, dist2, _ = h.search_batched(q, 10)
        assert h.stats()["fallback_pieces"] > 0
        np.testing.assert_array_equal(idx2, idx)
        np.testing.assert_array_equal(_bits(dist2), _bits(dist))
    finally:
        h.close()


@pytest.mark.parametrize("metric", [DOT, L2])
def test_fourfold_rows(oracle, metric):
    base, q = _data(1000, 100, 65, 21, metric)
    db = np.ascontiguousarray(np.tile(base, (4, 1)))
    h = _handle(db, metric)
    try:
        _check_batched(oracle, db, q, metric, 10, h.search_batched(q, 10))
        h.set_tuning(200, 16)
        _check_batched(oracle, db, q, metric, 10, h.search_batched(q, 10))
    finally:
        h.close()


def test_handle_reuse():
    db, q = _data(4097, 100, 130, 31, L2)
    h = _handle(db, L2)
    try:
        for nq, k in ((130, 100), (1, 1), (65, 256)):
            got = h.search_batched(q[:nq], k)
            fresh = _handle(db, L2)
            try:
                want = fresh.search_batched(q[:nq], k)
            finally:
                fresh.close()
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
            np.testing.assert_array_equal(got[2], want[2])
    finally:
        h.close()


def test_arguments():
    db, q = _data(100, 8, 4, 1, DOT)
    h = _handle(db, DOT)
    try:
        idx, dist, cnt = h.search_batched(q[:0], 10)     # nq == 0: SMX_OK, nothing written
        assert idx.shape == (0, 10)
        with pytest.raises(_native.SmxError, match="256"):
            h.search_batched(q, 257)
        with pytest.raises(_native.SmxError):
            h.search_batched(q, 0)
        with pytest.raises(_native.SmxError, match="dimsensionality"):
            h.search_batched(q[:, :7], 10)
        with pytest.raises(_native.SmxError):
            h.set_tuning(0, 5000)
    finally:
        h.close()


@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim", [100, 130])
def test_single_query(oracle, dim, metric):
    db, q = _data(3000, dim, 2, 50 + dim, metric)
    h = _handle(db, metric)
    try:
        for query in q:
            d = np.array([oracle.exact_distance(query, row, metric) for row in db], np.float32)
            order = np.lexsort((np.arange(db.shape[0]), d))[:10]
            idx, dist, cnt = h.search(query, 10)
            assert cnt == 10
            np.testing.assert_array_equal(idx, order.astype(np.uint32))
            np.testing.assert_array_equal(_bits(dist), _bits(d[order]))
        if dim == 100 and metric == DOT:
            # the reference's own test pins search == search_batched to 1e-6
            bi, bd, _ = h.search_batched(q, 10)
            for r, query in enumerate(q):
                _, sd, _ = h.search(query, 10)
                np.testing.assert_allclose(sd, bd[r], rtol=1e-6)
        # many passes and the overflow fallback in the one-to-many order
        h.set_tuning(100, 16)
        d = np.array([oracle.exact_distance(q[0], row, metric) for row in db], np.float32)
        order = np.lexsort((np.arange(db.shape[0]), d))[:10]
        idx, dist, _ = h.search(q[0], 10)
        np.testing.assert_array_equal(idx, order.astype(np.uint32))
        np.testing.assert_array_equal(_bits(dist), _bits(d[order]))
    finally:
        h.close()


@pytest.fixture(scope="module")
def uniform():
    """configs[0] scaled down: U[0,1), 10000 x 128, 100 queries, seed 1."""
    rng = np.random.default_rng(1)
    return rng.random((10000, 128), dtype=np.float32), rng.random((100, 128), dtype=np.float32)


def _exact64(db, q, idx, metric):
    x = db[idx.astype(np.int64)].astype(np.float64)
    qq = q.astype(np.float64)[:, None, :]
    return (x * qq).sum(-1) if metric == DOT else ((x - qq) ** 2).sum(-1)


def test_public_api_squared_l2(uniform, tmp_path):
    db, q = uniform
    s = scann_ops_pybind.builder(db, 10, "squared_l2").score_brute_force().build()
    assert s.size() == 10000
    idx, dist = s.search_batched(q)
    assert idx.shape == (100, 10) and dist.shape == (100, 10)
    truth = synthetic.brute_force_topk(db, q, 10, L2)
    assert synthetic.recall_at_k(idx.astype(np.int64), truth, 10) == 1.0
    np.testing.assert_allclose(dist, _exact64(db, q, idx, L2), rtol=1e-5)
    assert np.all(np.diff(dist, axis=1) >= 0)
    # pre_reorder_nn / leaves are accepted and ignored; parallel == batched
    pi, pd = s.search_batched_parallel(q, final_num_neighbors=10, pre_reorder_num_neighbors=50,
                                       leaves_to_search=7, batch_size=13)
    np.testing.assert_array_equal(pi, idx)
    np.testing.assert_array_equal(pd, dist)
    si, sd = s.search(q[0], final_num_neighbors=5)
    np.testing.assert_array_equal(si, idx[0, :5])
    np.testing.assert_allclose(sd, dist[0, :5], rtol=1e-5)
    # with docids, through serialize -> load_searcher
    docids = [f"doc{i}" for i in range(db.shape[0])]
    s2 = scann_ops_pybind.builder(db, 10, "squared_l2").score_brute_force().build(docids=docids)
    d = str(tmp_path / "bf")
    s2.serialize(d)
    back = scann_ops_pybind.load_searcher(d)
    li, ld = back.search_batched(q)
    assert li == [[docids[j] for j in row] for row in idx]
    np.testing.assert_array_equal(_bits(ld), _bits(dist))
    assert back.size() == 10000 and "brute_force" in back.config()


def test_public_api_dot_product(uniform):
    db, q = uniform
    s = scann_ops_pybind.builder(db, 10, "dot_product").score_brute_force().build()
    idx, dist = s.search_batched(q)
    truth = synthetic.brute_force_topk(db, q, 10, DOT)
    assert synthetic.recall_at_k(idx.astype(np.int64), truth, 10) == 1.0
    exact = _exact64(db, q, idx, DOT)
    assert np.all(exact > 0)
    np.testing.assert_allclose(dist, exact, rtol=1e-6)     # +dot, larger is better
    assert np.all(np.diff(dist, axis=1) <= 0)
