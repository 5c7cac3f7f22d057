"""GPU parity: every stage of the HIP path against the CPU oracle.

The bar (BASELINE.json north_star): neighbor ids bit-exact;
distances within 1e-4 relative -- the kernels in fact reproduce the oracle's
float bits, and the tests assert exact equality where the oracle fixes the
rounding, with the 1e-4 relative tolerance kept as the documented contract
(RTOL below) for the float outputs.
"""
import numpy as np
import pytest

from tests.conftest import make_index

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def native():
    from scann_amd import _native
    return _native


def _nat(native, ix):
    return native.NativeIndex(ix)


def test_partition_topl_bit_exact(native, oracle, small_dot, small_l2):
    for ix, db, q in (small_dot, small_l2):
        n = _nat(native, ix)
        for L in (1, 7, ix.num_leaves, ix.num_leaves + 5):
            gl, gd = n.partition_topl(q, L)
            ol, od = oracle.partition_topl(q, ix.centers, ix.metric, L)
            np.testing.assert_array_equal(gl, ol)
            np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_lookup_tables_bit_exact(native, oracle, small_dot, small_l2):
    for ix, db, q in (small_dot, small_l2):
        n = _nat(native, ix)
        lut, mult = n.create_lookup_tables(q)
        for i in range(q.shape[0]):
            _, u8, m = oracle.create_lut(q[i], ix.codebook, ix.metric)
            np.testing.assert_array_equal(lut[i], u8)
            assert np.float32(m).view(np.uint32) == mult[i].view(np.uint32)


def test_leaf_scores_exact(native, oracle, small_dot):
    ix, db, q = small_dot
    n = _nat(native, ix)
    lut, _ = n.create_lookup_tables(q[:3])
    for leaf in range(0, ix.num_leaves, 5):
        b, e = int(ix.leaf_offsets[leaf]), int(ix.leaf_offsets[leaf + 1])
        codes = ix.member_codes[b:e]
        for qi in range(3):
            got = n.leaf_scores(leaf, lut[qi])
            packed = oracle.pack_codes(codes) if e > b else np.zeros(0, np.uint8)
            want = oracle.lut16_accumulate(packed, e - b, ix.num_blocks, lut[qi]) if e > b else np.zeros(0, np.int32)
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("leaves,pre_nn", [(1, 10), (5, 50), (16, 100), (48, 200)])
def test_pre_reorder_matches_ideal_oracle(native, oracle, small_dot, leaves, pre_nn):
    ix, db, q = small_dot
    n = _nat(native, ix)
    gi, gd, gc = n.search_pre_reorder(q, leaves, pre_nn)
    oi, od, oc = oracle.search_pre_reorder(ix, q, leaves, pre_nn, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gc, oc)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_allclose(gd, od, rtol=RTOL, equal_nan=True)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("fix", ["small_dot", "small_l2"])
@pytest.mark.parametrize("reorder", [True, False])
def test_search_batched_matches_ideal_oracle(native, oracle, fix, reorder, request):
    ix, db, q = request.getfixturevalue(fix)
    n = _nat(native, ix)
    gi, gd, gc = n.search_batched(q, 12, 100, 10, reorder)
    oi, od, oc = oracle.search(ix, q, 12, 100, 10, reorder, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gc, oc)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_allclose(gd, od, rtol=RTOL, equal_nan=True)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_glove_shape_blocks_k25(native, oracle):
    """D=100, 2-dim blocks -> B=50, K=25: the glove kernel instantiation."""
    ix, db, q = make_index(n=20000, d=100, leaves=40, seed=3, components=80)
    n = _nat(native, ix)
    gi, gd, gc = n.search_batched(q, 8, 100, 10, True)
    oi, od, oc = oracle.search(ix, q, 8, 100, 10, True, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
    gi, gd, gc = n.search_pre_reorder(q, 8, 100)
    oi, od, oc = oracle.search_pre_reorder(ix, q, 8, 100, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_exact_distances_bit_exact(native, oracle, small_dot):
    ix, db, q = small_dot
    n = _nat(native, ix)
    rng = np.random.default_rng(0)
    ids = rng.integers(0, ix.num_datapoints, (q.shape[0], 17)).astype(np.uint32)
    got = n.exact_distances(q, ids)
    for i in range(q.shape[0]):
        for j in range(ids.shape[1]):
            want = oracle.exact_distance(q[i], db[ids[i, j]], ix.metric)
            assert np.float32(want).view(np.uint32) == got[i, j].view(np.uint32)


@pytest.mark.parametrize("chunk", [16, 32])
def test_overflow_tightening_is_exact(native, oracle, small_dot, chunk):
    """A tiny candidate capacity overflows every list: the device-side rescan
    (k'-th stored key as the new threshold) leaves the results unchanged."""
    ix, db, q = small_dot
    n = _nat(native, ix)
    n.set_tuning(128, 0, 0, chunk)   # no seed pass: every candidate is emitted -> overflow
    n.set_profiling(True)
    gi, gd, gc = n.search_pre_reorder(q, 48, 100)
    t = n.timings()
    assert t["overflow_retries"] >= 1
    oi, od, oc = oracle.search_pre_reorder(ix, q, 48, 100, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_soar_spilled_index_matches_oracle(native, oracle):
    """Datapoints in two leaves: k' = 2 x pre_nn before DeduplicateDatabaseSpilledResults."""
    from scann_amd import index_builder, synthetic
    db = synthetic.mixture(6000, 32, 48, 0.9, 41)
    q = synthetic.mixture(48, 32, 48, 0.9, 141, means_seed=41)
    ix = index_builder.build_tree_ah(db, 0, 40, 2, training_iterations=4,
                                     ah_training_iterations=4, soar_lambda=1.5, seed=41)
    assert not ix.disjoint
    n = _nat(native, ix)
    for leaves, pre in ((6, 20), (12, 100)):
        gi, gd, gc = n.search_pre_reorder(q, leaves, pre)
        oi, od, oc = oracle.search_pre_reorder(ix, q, leaves, pre, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gc, oc)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
        gi, gd, gc = n.search_batched(q, leaves, pre, 10, True)
        oi, od, oc = oracle.search(ix, q, leaves, pre, 10, True, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("metric,residual", [(1, False), (0, False)])
def test_soar_without_global_topn_matches_oracle(native, oracle, metric, residual):
    """SOAR spilling on an index without the global top-N tie (squared L2, or
    a non-residual dot index): both copies of a spilled datapoint carry the
    same codes, no bias and the global id as tie, so their keys coincide; the
    selection ranks equal keys stably (tree_x_hybrid_smmd.cc:784,
    DeduplicateDatabaseSpilledResults then averages the copies)."""
    from scann_amd import index_builder, synthetic
    db = synthetic.mixture(5000, 32, 40, 0.9, 43, normalize=metric == 0)
    q = synthetic.mixture(40, 32, 40, 0.9, 143, normalize=metric == 0, means_seed=43)
    ix = index_builder.build_tree_ah(db, metric, 30, 2, training_iterations=4,
                                     ah_training_iterations=4, soar_lambda=1.5,
                                     residual=residual, seed=43)
    assert not ix.disjoint
    n = _nat(native, ix)
    for leaves, pre in ((5, 20), (12, 100), (30, 128)):
        gi, gd, gc = n.search_pre_reorder(q, leaves, pre)
        oi, od, oc = oracle.search_pre_reorder(ix, q, leaves, pre, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gc, oc)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
        gi, gd, gc = n.search_batched(q, leaves, pre, 10, True)
        oi, od, oc = oracle.search(ix, q, leaves, pre, 10, True, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_edge_cases(native, oracle):
    """Empty leaves, a single query, k larger than the candidates available,
    leaves_to_search larger than num_leaves, duplicate vectors (ties)."""
    from scann_amd.index import TreeAHIndex
    ix, db, q = make_index(n=900, d=16, leaves=12, seed=9, components=10)
    # add an empty leaf and duplicated rows -> exact distance ties
    offsets = np.concatenate([ix.leaf_offsets, ix.leaf_offsets[-1:]])
    centers = np.concatenate([ix.centers, ix.centers[:1] + 5.0])
    ix2 = TreeAHIndex(metric=0, dim=16, num_blocks=ix.num_blocks, dims_per_block=2, residual=True,
                      centers=centers, codebook=ix.codebook, leaf_offsets=offsets,
                      leaf_members=ix.leaf_members, member_codes=ix.member_codes,
                      num_datapoints=ix.num_datapoints, dataset=ix.dataset)
    n = _nat(native, ix2)
    for nq, leaves, pre, final in ((1, 1, 5, 3), (7, 13, 50, 10), (5, 40, 2000, 25), (3, 2, 400, 400)):
        qq = q[:nq]
        gi, gd, gc = n.search_batched(qq, leaves, pre, final, True)
        oi, od, oc = oracle.search(ix2, qq, leaves, pre, final, True, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gc, oc)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(np.isnan(gd), np.isnan(od))
        np.testing.assert_array_equal(np.nan_to_num(gd).view(np.uint32), np.nan_to_num(od).view(np.uint32))
    # all-identical codes -> every distance ties inside a leaf
    codes = np.zeros_like(ix.member_codes)
    ix3 = TreeAHIndex(metric=0, dim=16, num_blocks=ix.num_blocks, dims_per_block=2, residual=True,
                      centers=ix.centers, codebook=ix.codebook, leaf_offsets=ix.leaf_offsets,
                      leaf_members=ix.leaf_members, member_codes=codes,
                      num_datapoints=ix.num_datapoints, dataset=None)
    n3 = _nat(native, ix3)
    gi, gd, gc = n3.search_pre_reorder(q, 5, 60)
    oi, od, oc = oracle.search_pre_reorder(ix3, q, 5, 60, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_errors_surface_as_status(native, small_dot):
    ix, db, q = small_dot
    n = _nat(native, ix)
    with pytest.raises(native.SmxError, match="dimsensionality"):
        n.search_batched(q[:, :16], 4, 10, 10)
    bad = q.copy()
    bad[0, 0] = np.nan
    with pytest.raises(native.SmxError, match="finite"):
        n.search_batched(bad, 4, 10, 10)


@pytest.mark.parametrize("chunk", [16, 32, 64, 200])
def test_scan_chunks_match_oracle(native, oracle, small_l2, chunk):
    """The scan at several work-item sizes (tiles per item)."""
    ix, db, q = small_l2
    n = _nat(native, ix)
    n.set_tuning(4096, 2, 0, chunk)
    gi, gd, gc = n.search_pre_reorder(q, 12, 60)
    oi, od, oc = oracle.search_pre_reorder(ix, q, 12, 60, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gc, oc)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_final_select_refinement_and_fallback(native, oracle):
    """No seed threshold, so every scanned datapoint is a candidate (n well
    above the rank select's 256-key buffer): its histogram refinement runs for
    every query, and for queries next to a block of 1200 identical datapoints
    one distance value holds > 256 keys, which sends them to the exact radix
    select over whole keys.  Both must equal the ideal oracle."""
    from scann_amd import index_builder, synthetic
    db = synthetic.mixture(3000, 16, 8, 0.9, 7)
    db[:1200] = db[0]
    rng = np.random.default_rng(7)
    near = db[:6] + np.float32(0.01) * rng.standard_normal((6, 16)).astype(np.float32)
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    q = np.concatenate([near, synthetic.mixture(10, 16, 8, 0.9, 107, means_seed=7)]).astype(np.float32)
    ix = index_builder.build_tree_ah(db, 0, 6, 2, training_iterations=4,
                                     ah_training_iterations=4, seed=7)
    n = _nat(native, ix)
    n.set_tuning(4096, 0)
    for leaves, pre in ((6, 100), (3, 40)):
        gi, gd, gc = n.search_pre_reorder(q, leaves, pre)
        oi, od, oc = oracle.search_pre_reorder(ix, q, leaves, pre, oracle.MODE_IDEAL)
        np.testing.assert_array_equal(gc, oc)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
    gi, gd, gc = n.search_batched(q, 6, 100, 10, True)
    oi, od, oc = oracle.search(ix, q, 6, 100, 10, True, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("pre_nn", [300, 2000])
def test_large_kprime_block_select(native, oracle, small_dot, pre_nn):
    """k' above the rank kernel's 256 keys (the block select kernel), up to
    the supported maximum 2048 (ADVICE: a case near k' max)."""
    ix, db, q = small_dot
    n = _nat(native, ix)
    gi, gd, gc = n.search_pre_reorder(q, 24, pre_nn)
    oi, od, oc = oracle.search_pre_reorder(ix, q, 24, pre_nn, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gc, oc)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
    gi, gd, gc = n.search_batched(q, 24, pre_nn, 10, True)
    oi, od, oc = oracle.search(ix, q, 24, pre_nn, 10, True, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_allclose(gd, od, rtol=RTOL)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_overflow_rescan_in_block_select(native, oracle, small_dot):
    """k' = 300 with a 600-key list and no seed threshold: every list
    overflows and the block select kernel rescans it on the device."""
    ix, db, q = small_dot
    n = _nat(native, ix)
    n.set_tuning(600, 0, 0, 32)
    n.set_profiling(True)
    gi, gd, gc = n.search_pre_reorder(q, 48, 300)
    assert n.timings()["overflow_retries"] >= 1
    oi, od, oc = oracle.search_pre_reorder(ix, q, 48, 300, oracle.MODE_IDEAL)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_device_entry_point_is_stream_ordered(native, oracle, small_dot):
    """search_batched_device returns with the work enqueued on torch's
    current stream (no host synchronisation inside): back-to-back calls into
    different output buffers, read after the stream, equal the oracle."""
    import torch
    ix, db, q = small_dot
    n = _nat(native, ix)
    qd = torch.from_numpy(q).cuda()
    outs = []
    for _ in range(3):
        oi_ = torch.full((q.shape[0], 10), -1, dtype=torch.int32, device="cuda")
        od_ = torch.zeros((q.shape[0], 10), dtype=torch.float32, device="cuda")
        n.search_batched_device(qd.data_ptr(), q.shape[0], 12, 100, 10, True, oi_.data_ptr(),
                                od_.data_ptr())
        outs.append((oi_, od_))
    oi, od, oc = oracle.search(ix, q, 12, 100, 10, True, oracle.MODE_IDEAL)
    for oi_, od_ in outs:
        np.testing.assert_array_equal(oi_.cpu().numpy().view(np.uint32), oi)
        np.testing.assert_allclose(od_.cpu().numpy(), od, rtol=RTOL)
        np.testing.assert_array_equal(od_.cpu().numpy().view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("fix", ["small_dot", "small_l2"])
@pytest.mark.parametrize("reorder", [False, True])
def test_single_query_search_matches_oracle(native, oracle, fix, reorder, request):
    """f4: search() (smx_search) scores partitions in the single-query
    one-to-many order; against the oracle's PARTITION_ONE_TO_MANY mode the
    ids and distance bits agree (without reorder the distances carry the
    leaf biases, so the biases are pinned too)."""
    ix, db, q = request.getfixturevalue(fix)
    n = _nat(native, ix)
    mode = oracle.MODE_IDEAL | oracle.PARTITION_ONE_TO_MANY
    for i in range(12):
        gi, gd, gc = n.search(q[i], 12, 100, 10, reorder)
        oi, od, oc = oracle.search(ix, q[i:i + 1], 12, 100, 10, reorder, mode)
        assert gc == int(oc[0])
        np.testing.assert_array_equal(gi[:gc], oi[0, :gc])
        np.testing.assert_array_equal(gd[:gc].view(np.uint32), od[0, :gc].view(np.uint32))


