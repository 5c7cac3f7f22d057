"""Host side of the brute-force searcher (no GPU): the config reader and its
dispatch, the asset round trip of a brute-force searcher, and the conditions
the shapes of test_gpu_brute_force_paths.py rely on (which kernel paths they
reach, that the reference keeps them off the overflow fallback, that the
subnormal data is subnormal)."""
import json
import os
import re

import numpy as np
import pytest

from scann_amd import assets, config
from scann_amd.brute_force import BruteForceIndex
from scann_amd.index import METRIC_DOT, METRIC_SQUARED_L2
from tests import test_gpu_brute_force_paths as paths
from tests.conftest import ROOT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builder_configs.json")


@pytest.fixture(scope="module")
def golden_text():
    with open(GOLDEN) as f:
        cases = {c["name"]: c for c in json.load(f)}
    return cases["brute_force"]["config"]


def test_golden_config_parses(golden_text):
    cfg = config.brute_force_config_from_text(golden_text)
    assert cfg == config.BruteForceConfig(num_neighbors=3, metric="squared_l2")
    assert config.is_brute_force(config.parse_text_proto(golden_text))


def test_tree_ah_reader_still_rejects(golden_text):
    with pytest.raises(ValueError, match="score_brute_force"):
        config.search_config_from_text(golden_text)


HEAD = 'num_neighbors: 3\ndistance_measure {distance_measure: "DotProductDistance"}\n'


@pytest.mark.parametrize("body", [
    "brute_force { fixed_point { enabled: true } }",
    "brute_force { bfloat16 { enabled: true } }",
    "partitioning { num_children: 10 }\nbrute_force { fixed_point { enabled: false } }",
])
def test_unsupported_brute_force_rejected(body):
    with pytest.raises(ValueError):
        config.brute_force_config_from_text(HEAD + body)


def test_plain_variants_accepted():
    for body in ("brute_force { fixed_point { enabled: false } }",
                 "brute_force { bfloat16 { enabled: False } }"):
        cfg = config.brute_force_config_from_text(HEAD + body)
        assert cfg == config.BruteForceConfig(num_neighbors=3, metric="dot_product")


def test_not_a_brute_force_config():
    with pytest.raises(ValueError):
        config.brute_force_config_from_text(HEAD)


@pytest.mark.parametrize("relative", [False, True])
def test_asset_round_trip(tmp_path, golden_text, relative):
    rng = np.random.default_rng(5)
    db = rng.standard_normal((37, 5)).astype(np.float32)
    db[3, 2] = -0.0
    index = BruteForceIndex(db, METRIC_SQUARED_L2)
    d = str(tmp_path / "bf")
    text = assets.save_brute_force_artifacts(index, golden_text, d, relative)
    assert sorted(os.listdir(d)) == ["dataset.npy", "scann_assets.pbtxt", "scann_config.pb"]
    assert "DATASET_NPY" in text
    assert assets.is_brute_force_artifacts(d)
    back, tree, cfg = assets.load_brute_force_artifacts(d)
    assert back.metric == METRIC_SQUARED_L2 and back.dim == 5 and back.num_datapoints == 37
    assert np.array_equal(back.dataset.view(np.uint32), db.view(np.uint32))
    assert cfg == config.brute_force_config_from_text(golden_text)
    # the decoded config prints as a config that parses to the same thing
    assert config.brute_force_config_from_text(assets.config_text(tree)) == cfg
    # the asset list passed explicitly, as ScannNumpy(artifacts_dir, assets_pbtxt) does
    again, _, _ = assets.load_brute_force_artifacts(d, text)
    assert np.array_equal(again.dataset, db)


def test_index_desc_and_checks():
    db = np.arange(12, dtype=np.float64).reshape(4, 3)
    index = BruteForceIndex(db, METRIC_DOT)
    assert index.dataset.dtype == np.float32 and index.dataset.flags.c_contiguous
    desc = index.desc()
    assert (desc.metric, desc.dim, desc.num_datapoints) == (METRIC_DOT, 3, 4)
    assert desc.dataset == index.dataset.ctypes.data
    with pytest.raises(ValueError):
        BruteForceIndex(np.zeros(3, np.float32), METRIC_DOT)
    with pytest.raises(ValueError):
        BruteForceIndex(np.zeros((2, 3), np.float32), 7)


def test_tree_ah_artifacts_are_not_brute_force(tmp_path):
    tree_cfg = HEAD + "partitioning { num_children: 10 }\n"
    d = tmp_path / "ah"
    d.mkdir()
    with open(d / "scann_config.pb", "wb") as f:
        f.write(assets.encode_message(config.parse_text_proto(tree_cfg), "ScannConfig"))
    assert not assets.is_brute_force_artifacts(str(d))


# ---- the shapes of test_gpu_brute_force_paths.py ------------------------------
DOT, L2 = METRIC_DOT, METRIC_SQUARED_L2


def test_schedule_model_matches_the_source():
    """The constants the host model restates are those of the kernels' file."""
    with open(os.path.join(ROOT, "scann_amd", "csrc", "smx_brute_force.hip")) as f:
        src = f.read()

    def const(name):
        m = re.search(r"\b%s = ([0-9]+)( << ([0-9]+))?[,;]" % name, src)
        return int(m.group(1)) << int(m.group(3) or 0)

    assert const("kBfTile") == paths.TILE and const("kBfBlocks") == paths.BLOCKS
    assert const("kBfGrowth") == paths.GROWTH and const("kBfMaxPassRows") == paths.MAX_PASS_ROWS
    assert const("kBfMaxBatch") == paths.MAX_BATCH
    assert (const("kBfCapMax"), const("kBfFullDim")) == (3840, 128)
    assert [paths.default_cap(k) for k in (1, 10, 64, 100, 256)] == [1024, 1024, 1024, 1600, 3840]


def test_schedule_model_known_values():
    m = paths.MULTI
    slabs = paths.pass_schedule(m["n"], m["first"], paths.default_cap(10))
    assert slabs == [(0, 1000), (1000, 5000), (5000, 12500)]
    assert [paths.launch_shape(m["nq"], *s) for s in slabs] == [
        (18, 16, 1, 16), (18, 63, 2, 32), (18, 118, 3, 40)]
    c = paths.PASS_CAP
    slabs = paths.pass_schedule(c["n"], 0, paths.default_cap(c["k"]))
    assert [b - a for a, b in slabs] == [1024, 4096, 16384, 65536, 262144, 1048576,
                                         4194304, 4194304, 1000]
    assert paths.launch_shape(c["nq"], *slabs[6]) == (1, 65536, 64, 1024)
    assert paths.pass_schedule(5, 0, 1024) == [(0, 5)]
    assert paths.pass_schedule(20000, 128, 1024)[-1] == (10880, 20000)


def test_shapes_reach_every_path():
    """What the GPU cases are named for, from the model: per row-tile count,
    short last blocks, partial last tiles, unaligned first rows -- for the
    full-dim kernel (dim <= 128) and the chunked one."""
    m, c = paths.MULTI, paths.PASS_CAP
    reached = {"full": [], "chunked": []}
    for dim, k in paths.MULTI_CASES:
        for row0, row1 in paths.pass_schedule(m["n"], m["first"], paths.default_cap(k)):
            reached["full" if dim <= 128 else "chunked"].append(
                (row0, row1) + paths.launch_shape(m["nq"], row0, row1))
    for row0, row1 in paths.pass_schedule(c["n"], 0, paths.default_cap(c["k"])):
        assert c["dim"] <= 128
        reached["full"].append((row0, row1) + paths.launch_shape(c["nq"], row0, row1))

    def short_last_block(s):
        return s[4] > 1 and s[3] % s[4] != 0

    def partial_last_tile(s):
        return s[4] > 1 and (s[1] - s[0]) % paths.TILE != 0

    for kernel in ("full", "chunked"):
        shapes = reached[kernel]
        assert any(s[4] == 2 for s in shapes), kernel
        assert any(s[4] >= 3 for s in shapes), kernel
        assert any(short_last_block(s) for s in shapes), kernel
        assert any(partial_last_tile(s) for s in shapes), kernel
        assert any(s[4] > 1 and s[0] % paths.TILE != 0 for s in shapes), kernel
        # a multi-tile pass is never the first (open thresholds: every row a candidate)
        assert all(s[4] == 1 for s in shapes if s[0] == 0), kernel
    assert sum(s[4] == 64 and s[1] - s[0] == paths.MAX_PASS_ROWS for s in reached["full"]) == 2
    assert {k for d, k in paths.MULTI_CASES if d <= 128} == {10, 100, 256}
    # sub-batches: a full one and a second with a partial query tile, one pass each
    sb = paths.SUB_BATCH
    assert paths.MAX_BATCH < sb["nq"] < 2 * paths.MAX_BATCH and (sb["nq"] - paths.MAX_BATCH) % 64
    assert len(paths.pass_schedule(sb["n"], 0, paths.default_cap(sb["k"]))) == 1
    # subnormals: two passes by default, four with the fallback's tuning
    sn = paths.SUBNORMAL
    assert len(paths.pass_schedule(sn["n"], 0, paths.default_cap(sn["k"]))) == 2
    assert len(paths.pass_schedule(sn["n"], 100, 16)) == 4


def _scores64(db, q, metric):
    x, y = db.astype(np.float64), q.astype(np.float64)
    dots = y @ x.T
    if metric == DOT:
        return -dots
    return (y * y).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * dots


def _chain_error_bound(db, q, metric):
    """Per query, what the float32 chain of dim fused steps (and, for squared
    L2, the two rounded norms it starts from) can differ by from the exact
    score: (dim + 2) 2^-24 times the sum of the terms' magnitudes, bounded by
    |q| |x| (dot) or (|q| + |x|)^2 (squared L2) with the largest row norm."""
    dim = db.shape[1]
    xn = np.sqrt((db.astype(np.float64) ** 2).sum(1)).max()
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(1))
    mags = qn * xn if metric == DOT else (qn + xn) ** 2
    return (dim + 2) * 2.0 ** -24 * mags


def _largest_counts(scores, slack, k, slabs):
    """Per later pass, the largest per-query number of its rows at or under
    the k-th score of the rows before it (+ slack)."""
    out = []
    for row0, row1 in slabs[1:]:
        tau = np.partition(scores[:, :row0], k - 1, axis=1)[:, k - 1] + slack
        out.append(int((scores[:, row0:row1] <= tau[:, None]).sum(1).max()))
    return out


@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim", sorted({d for d, _ in paths.MULTI_CASES}))
def test_multi_tile_cases_stay_off_the_fallback(dim, metric):
    """In float64, with twice the chain's rounding bound as slack (threshold
    and score may both be off): no query has more than cap / 2 candidates in
    a pass of the multi-tile cases, so their results are the MFMA kernel's."""
    m = paths.MULTI
    db, q = paths.multi_data(dim, metric)
    scores = _scores64(db, q, metric)
    slack = 2.0 * _chain_error_bound(db, q, metric)
    for k in sorted(k for d, k in paths.MULTI_CASES if d == dim):
        cap = paths.default_cap(k)
        slabs = paths.pass_schedule(m["n"], m["first"], cap)
        counts = _largest_counts(scores, slack, k, slabs)
        print("dim", dim, "metric", metric, "k", k, "largest counts", counts, "cap", cap)
        assert slabs[0][1] <= cap
        assert all(c <= cap // 2 for c in counts)


def _dim1_scores32(db, q, metric):
    """The batched chain at dim 1, a single fused step, in numpy: the product
    of two floats is exact in float64, so one rounding to float32 remains
    (squared L2: up to a second rounding of the float64 difference, which the
    comparison with the oracle below would show in the top k)."""
    x, y = db[:, 0], q[:, 0]
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    if metric == DOT:
        return (-(y64[:, None] * x64[None, :])).astype(np.float32) + np.float32(0)
    xnorm = x * x                                   # float32, rounded once
    qnorm = (y64 * y64).astype(np.float32)
    start = qnorm[:, None] + xnorm[None, :]         # float32 add
    return (start.astype(np.float64) - y64[:, None] * (2.0 * x64)[None, :]).astype(np.float32) \
        + np.float32(0)


@pytest.mark.parametrize("metric", [DOT, L2])
def test_pass_cap_case_stays_off_the_fallback(oracle, metric):
    """Float64 with a rounding bound says nothing at dim 1 and 9.8 M rows (the
    rows within rounding of a query outnumber cap), so the reference's own
    float32 scores are restated, checked against the oracle's top k, and the
    candidates counted exactly, ties included."""
    c = paths.PASS_CAP
    k, cap = c["k"], paths.default_cap(c["k"])
    db, q = paths.pass_cap_data(metric)
    scores = _dim1_scores32(db, q, metric)
    oi, od = oracle.partition_topl(q, db, metric, k)
    for r in range(c["nq"]):
        order = np.lexsort((np.arange(c["n"]), scores[r]))[:k]
        np.testing.assert_array_equal(order, oi[r])
        np.testing.assert_array_equal(scores[r][order].view(np.uint32), od[r].view(np.uint32))
    slabs = paths.pass_schedule(c["n"], 0, cap)
    counts = _largest_counts(scores, np.zeros(c["nq"], np.float32), k, slabs)
    print("metric", metric, "largest counts", counts, "cap", cap)
    assert len(slabs) == 9 and slabs[0][1] <= cap
    assert all(n <= cap // 2 for n in counts)


@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim", [100, 130])
@pytest.mark.parametrize("scaling", sorted(paths.SCALINGS))
def test_subnormal_cases_are_subnormal(oracle, scaling, dim, metric):
    tiny = np.finfo(np.float32).tiny
    k = paths.SUBNORMAL["k"]
    db, q = paths.subnormal_data(dim, metric, scaling)
    _, od = oracle.partition_topl(q, db, metric, k)
    one = np.array([[oracle.exact_distance(query, row, metric) for row in db] for query in q[:2]],
                   np.float32)
    if scaling == "scores":
        # every top-k score of both orders a nonzero subnormal (a dot product
        # of the other rows may round to zero: under 1 % of them do)
        assert np.all(od != 0) and np.all(np.abs(od) < tiny)
        top = np.sort(one, axis=1)[:, :k]
        assert np.all(top != 0) and np.all(np.abs(one) < tiny) and np.mean(one != 0) > 0.99
    else:
        # every row entry below the normal range (a few round to zero), the
        # queries normal, and the scores not flushed away
        assert np.all(np.abs(db) < tiny) and np.mean(db != 0) > 0.99
        assert np.all(np.abs(q[q != 0]) >= tiny)
        assert np.any(od != 0) and np.any(one != 0)
        if metric == DOT:
            assert np.all(od != 0) and len(np.unique(od)) > od.size // 2
        else:
            # all rows tie at |q|^2 (see test_subnormals)
            assert np.all(od == od[:, :1])
