"""The exact brute-force searcher on the paths its benchmark runs on
(scann_amd/csrc/smx_brute_force.hip): several row tiles per block, the device
entry point, sub-batches above 8192 queries, workspace growth on a live
handle, the capped pass size and subnormal scores and operands.

References as in test_gpu_brute_force.py: oracle.partition_topl with the
database as centers (batched) and oracle.exact_distance per row (single
query); ids, counts and distance bits must be equal.

pass_schedule / launch_shape / default_cap restate RunBf's host arithmetic;
every GPU test ties them to the library through stats()["passes"], and
test_brute_force_host.py asserts from them that the shapes below reach the
paths they are named for."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests.test_gpu_brute_force import DOT, L2, _bits, _check_batched, _data, _handle

gpu = pytest.mark.gpu

TILE, BLOCKS, GROWTH, MAX_PASS_ROWS, MAX_BATCH = 64, 1024, 4, 1 << 22, 8192


# ---- the host model of RunBf ------------------------------------------------
def default_cap(k):
    return min(3840, max(1024, 16 * k))


def pass_schedule(n, first_pass_rows, cap):
    """The (row0, row1) slabs of one call."""
    size, row0, out = first_pass_rows or cap, 0, []
    while row0 < n:
        row1 = min(n, row0 + size)
        out.append((row0, row1))
        row0, size = row1, min(MAX_PASS_ROWS, size * GROWTH)
    return out


def launch_shape(nq, row0, row1):
    """(qtiles, ctl, per, grid_y) of bf_pass_kernel over rows [row0, row1)."""
    qtiles = -(-nq // TILE)
    ctl = -(-(row1 - row0) // TILE)
    per = max(1, -(-(qtiles * ctl) // BLOCKS))
    return qtiles, ctl, per, -(-ctl // per)


# ---- the shapes ---------------------------------------------------------------
# several row tiles per block: 18 query tiles, passes [0, 1000) (per 1),
# [1000, 5000) (per 2) and [5000, 12500) (per 3, a last tile of 12 rows)
MULTI = dict(nq=1100, n=12500, first=1000, seed=5)
MULTI_CASES = [(100, 10), (100, 100), (100, 256), (130, 10)]   # dim, k
# the pass size capped at 2^22: 1024, 4096, ..., 2^22, 2^22, 1000 rows
PASS_CAP = dict(n=9787368, dim=1, nq=3, k=10, seed=41)
SUB_BATCH = dict(nq=MAX_BATCH + 65, n=300, dim=8, k=10)
SUBNORMAL = dict(n=3000, nq=65, k=10)
# (rows, queries) scaled by 2^a, 2^b: "scores" makes every score a nonzero
# subnormal (the MFMA's C/D), "operand" the rows themselves (its B)
SCALINGS = {"scores": (-70, -70), "operand": (-135, 10)}


def multi_data(dim, metric):
    return _data(MULTI["n"], dim, MULTI["nq"], MULTI["seed"], metric)


def pass_cap_data(metric):
    return _data(PASS_CAP["n"], PASS_CAP["dim"], PASS_CAP["nq"], PASS_CAP["seed"] + metric, metric)


def subnormal_data(dim, metric, scaling):
    db, q = _data(SUBNORMAL["n"], dim, SUBNORMAL["nq"], 600 + dim + metric, metric)
    a, b = SCALINGS[scaling]
    return np.ldexp(db, a).astype(np.float32), np.ldexp(q, b).astype(np.float32)


def one_to_many(oracle, db, query, metric, k):
    """(ids, distances) of the single-query reference."""
    d = np.array([oracle.exact_distance(query, row, metric) for row in db], np.float32)
    order = np.lexsort((np.arange(db.shape[0]), d))[:k]
    return order.astype(np.uint32), d[order]


class _Memo:
    """oracle.partition_topl, each distinct call computed once for the module
    and handed out read-only."""

    def __init__(self):
        self.oracle, self.seen = None, {}

    def partition_topl(self, q, db, metric, k):
        key = (q.shape, db.shape, metric, k, hashlib.sha1(q.tobytes()).digest(),
               hashlib.sha1(db.tobytes()).digest())
        if key not in self.seen:
            oi, od = self.oracle.partition_topl(q, db, metric, k)
            oi.flags.writeable = od.flags.writeable = False
            self.seen[key] = (oi, od)
        return self.seen[key]


_MEMO = _Memo()


@pytest.fixture()
def ref(oracle):
    _MEMO.oracle = oracle
    return _MEMO


def _check_passes(h, n, first, cap):
    st = h.stats()
    print("stats", st)
    assert st["passes"] == len(pass_schedule(n, first, cap))
    return st


# ---- 1. several row tiles per block ----------------------------------------
@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim,k", MULTI_CASES)
def test_multi_tile_blocks(ref, dim, k, metric):
    """The prefetch beside the MFMAs, the barrier before cs is overwritten,
    the per-tile init_acc and ct_end of a short last block, on the MFMA path:
    no query overflows its buffer, so no pass is rescored by the fold."""
    db, q = multi_data(dim, metric)
    h = _handle(db, metric)
    try:
        h.set_tuning(MULTI["first"], 0)
        got = h.search_batched(q, k)
        st = _check_passes(h, MULTI["n"], MULTI["first"], default_cap(k))
        assert st["fallback_pieces"] == 0
        assert st["max_candidates"] <= default_cap(k)
        _check_batched(ref, db, q, metric, k, got)
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_multi_tile_blocks_with_overflow(ref, metric):
    """64 candidates a query: the multi-tile passes overflow for most queries
    and the fold rescores them."""
    db, q = multi_data(100, metric)
    h = _handle(db, metric)
    try:
        h.set_tuning(MULTI["first"], 64)
        got = h.search_batched(q, 10)
        st = _check_passes(h, MULTI["n"], MULTI["first"], 64)
        assert st["fallback_pieces"] > 0 and st["max_candidates"] > 64
        _check_batched(ref, db, q, metric, 10, got)
    finally:
        h.close()


# ---- 2. the device entry point ----------------------------------------------
# A call is enqueued on the stream it is given.  torch's default stream has
# the handle 0, which the C ABI reads as "the handle's own stream", so the
# tests below order their buffers' fills before the calls with one device
# synchronisation and wait for a call's results through its stream (the
# device for the default stream).
IDX_FILL, DIST_FILL, COUNT_FILL = -1, -7.0, -3


class _DeviceBuffers:
    def __init__(self, torch, q, k, count=True):
        nq = q.shape[0]
        self.k = k
        self.q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        self.idx = torch.full((nq, k), IDX_FILL, dtype=torch.int32, device="cuda")
        self.dist = torch.full((nq, k), DIST_FILL, dtype=torch.float32, device="cuda")
        self.count = torch.full((nq,), COUNT_FILL, dtype=torch.int32, device="cuda") if count else None

    def call(self, h, stream=None, k=None):
        h.search_batched_device(self.q.data_ptr(), self.q.shape[0], self.k if k is None else k,
                                self.idx.data_ptr(), self.dist.data_ptr(),
                                None if self.count is None else self.count.data_ptr(),
                                stream=None if stream is None else ctypes.c_void_p(stream.cuda_stream))

    def result(self, n):
        idx = self.idx.cpu().numpy().view(np.uint32)
        dist = self.dist.cpu().numpy()
        cnt = (np.full(idx.shape[0], min(self.k, n), np.int32) if self.count is None
               else self.count.cpu().numpy())
        return idx, dist, cnt


@pytest.fixture(scope="module")
def dev_data():
    """N = 4097, dim 100, three sets of 130 queries, per metric."""
    out = {}
    for metric in (DOT, L2):
        db, q = _data(4097, 100, 390, 88 + metric, metric)
        out[metric] = (db, [np.ascontiguousarray(q[i * 130:(i + 1) * 130]) for i in range(3)])
    return out


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("where", ["default", "current", "explicit"])
def test_device_entry_point(ref, dev_data, where, metric):
    """On torch's default stream, on a non-default current stream and on a
    stream passed explicitly, with and without a count buffer."""
    import torch
    db, qs = dev_data[metric]
    q = qs[0]
    side = torch.cuda.Stream()
    h = _handle(db, metric)
    try:
        for k, count in ((10, True), (100, False)):
            buf = _DeviceBuffers(torch, q, k, count)
            torch.cuda.synchronize()
            if where == "default":
                buf.call(h)
                torch.cuda.synchronize()
            elif where == "current":
                with torch.cuda.stream(side):
                    buf.call(h)
                side.synchronize()
            else:
                buf.call(h, side)
                side.synchronize()
            _check_batched(ref, db, q, metric, k, buf.result(db.shape[0]))
            _check_passes(h, db.shape[0], 0, default_cap(k))
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_device_entry_point_pads(ref, metric):
    """k > N: counts of N, id 0 / NaN behind them."""
    import torch
    db, q = _data(5, 100, 33, 17 + metric, metric)
    side = torch.cuda.Stream()
    h = _handle(db, metric)
    try:
        buf = _DeviceBuffers(torch, q, 10)
        torch.cuda.synchronize()
        buf.call(h, side)
        side.synchronize()
        got = buf.result(5)
        assert np.all(got[2] == 5)
        _check_passes(h, 5, 0, default_cap(10))
        _check_batched(ref, db, q, metric, 10, got)
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_device_calls_are_stream_ordered(ref, dev_data, metric):
    """Three calls back to back on one stream, different queries and output
    buffers, no synchronisation between them: one workspace, used in stream
    order."""
    import torch
    db, qs = dev_data[metric]
    side = torch.cuda.Stream()
    h = _handle(db, metric)
    try:
        bufs = [_DeviceBuffers(torch, q, k) for q, k in zip(qs, (10, 100, 10))]
        torch.cuda.synchronize()
        for buf in bufs:
            buf.call(h, side)
        side.synchronize()
        _check_passes(h, db.shape[0], 0, default_cap(bufs[-1].k))
        for buf, q in zip(bufs, qs):
            _check_batched(ref, db, q, metric, buf.k, buf.result(db.shape[0]))
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_stream_change_and_host_call(ref, dev_data, metric):
    """Stream A, at once stream B (the handle waits for A before it reuses the
    workspace), at once the host-buffer call."""
    import torch
    db, qs = dev_data[metric]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    h = _handle(db, metric)
    try:
        ba, bb = _DeviceBuffers(torch, qs[0], 100), _DeviceBuffers(torch, qs[1], 10, count=False)
        torch.cuda.synchronize()
        ba.call(h, a)
        bb.call(h, b)
        host = h.search_batched(qs[2], 100)
        a.synchronize()
        b.synchronize()
        _check_passes(h, db.shape[0], 0, default_cap(100))
        _check_batched(ref, db, qs[0], metric, 100, ba.result(db.shape[0]))
        _check_batched(ref, db, qs[1], metric, 10, bb.result(db.shape[0]))
        _check_batched(ref, db, qs[2], metric, 100, host)
    finally:
        h.close()


@gpu
def test_device_entry_point_arguments(dev_data):
    import torch
    from scann_amd import _native
    db, qs = dev_data[DOT]
    side = torch.cuda.Stream()
    h = _handle(db, DOT)
    try:
        buf = _DeviceBuffers(torch, qs[0], 10)
        torch.cuda.synchronize()
        # nq == 0: SMX_OK, nothing written
        h.search_batched_device(buf.q.data_ptr(), 0, 10, buf.idx.data_ptr(), buf.dist.data_ptr(),
                                buf.count.data_ptr(), stream=ctypes.c_void_p(side.cuda_stream))
        with pytest.raises(_native.SmxError):
            buf.call(h, side, k=0)
        with pytest.raises(_native.SmxError, match="256"):
            buf.call(h, side, k=257)
        side.synchronize()
        torch.cuda.synchronize()
        assert bool((buf.idx == IDX_FILL).all()) and bool((buf.dist == DIST_FILL).all())
        assert bool((buf.count == COUNT_FILL).all())
    finally:
        h.close()


# ---- 3. sub-batches ---------------------------------------------------------------
@pytest.fixture(scope="module")
def sub_batch_data():
    c = SUB_BATCH
    return {m: _data(c["n"], c["dim"], c["nq"], 300 + m, m) for m in (DOT, L2)}


@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_sub_batches(ref, sub_batch_data, entry, metric):
    """8192 + 65 queries: two RunBf calls over one workspace, outputs offset by
    b * k and counts by b; equal to the oracle and to two separate calls."""
    import torch
    db, q = sub_batch_data[metric]
    n, k = SUB_BATCH["n"], SUB_BATCH["k"]
    side = torch.cuda.Stream()

    def search(h, qq):
        if entry == "host":
            return h.search_batched(qq, k)
        buf = _DeviceBuffers(torch, qq, k)
        torch.cuda.synchronize()
        buf.call(h, side)
        side.synchronize()
        return buf.result(n)

    h = _handle(db, metric)
    try:
        got = search(h, q)
        _check_passes(h, n, 0, default_cap(k))
        _check_batched(ref, db, q, metric, k, got)
        parts = [search(h, q[:MAX_BATCH]), search(h, q[MAX_BATCH:])]
        idx, dist, cnt = (np.concatenate(x) for x in zip(*parts))
        np.testing.assert_array_equal(idx, got[0])
        np.testing.assert_array_equal(_bits(dist), _bits(got[1]))
        np.testing.assert_array_equal(cnt, got[2])
    finally:
        h.close()


# ---- 4. growth on a live handle --------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_workspace_growth(ref, metric):
    """nq 1 -> 130 -> 65 -> 8257 -> 130 on one handle, host and device calls
    mixed: the workspace and the host calls' staging buffers are freed and
    reallocated under a handle that has already searched."""
    import torch
    n, dim = 3000, 16
    db, q = _data(n, dim, MAX_BATCH + 65, 400 + metric, metric)
    side = torch.cuda.Stream()

    def search(h, nq, k, entry):
        if entry == "host":
            return h.search_batched(q[:nq], k)
        buf = _DeviceBuffers(torch, q[:nq], k)
        torch.cuda.synchronize()
        buf.call(h, side)
        side.synchronize()
        return buf.result(n)

    h = _handle(db, metric)
    try:
        for nq, k, entry in ((1, 1, "host"), (130, 100, "host"), (65, 256, "device"),
                             (MAX_BATCH + 65, 10, "host"), (130, 100, "device")):
            got = search(h, nq, k, entry)
            _check_passes(h, n, 0, default_cap(k))
            _check_batched(ref, db, q[:nq], metric, k, got)
            fresh = _handle(db, metric)
            try:
                want = search(fresh, nq, k, entry)
            finally:
                fresh.close()
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
            np.testing.assert_array_equal(got[2], want[2])
    finally:
        h.close()


# ---- 5. the pass cap --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
def test_pass_cap(ref, metric):
    """9 787 368 rows of one dim: the seventh and eighth pass take 2^22 rows
    each (not 2^24), 64 row tiles per block."""
    c = PASS_CAP
    db, q = pass_cap_data(metric)
    h = _handle(db, metric)
    try:
        got = h.search_batched(q, c["k"])
        st = _check_passes(h, c["n"], 0, default_cap(c["k"]))
        assert st["passes"] == 9
        assert st["fallback_pieces"] == 0 and st["max_candidates"] <= default_cap(c["k"])
        _check_batched(ref, db, q, metric, c["k"], got)
    finally:
        h.close()


# ---- 6. subnormals ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", [DOT, L2])
@pytest.mark.parametrize("dim", [100, 130])
@pytest.mark.parametrize("scaling", sorted(SCALINGS))
def test_subnormals(oracle, ref, scaling, dim, metric):
    """Subnormal scores ("scores") and subnormal rows ("operand") through the
    MFMA kernels, the fold's scalar rescoring and the one-to-many search: a
    flush to zero anywhere changes bits or order."""
    n, k = SUBNORMAL["n"], SUBNORMAL["k"]
    db, q = subnormal_data(dim, metric, scaling)
    # squared L2 of subnormal rows: |x|^2 is 0 and 2 q.x below half an ulp of
    # |q|^2, so every row ties at |q|^2 and overflows the buffer by design
    all_tie = scaling == "operand" and metric == L2
    h = _handle(db, metric)
    try:
        got = h.search_batched(q, k)
        st = _check_passes(h, n, 0, default_cap(k))
        if not all_tie:
            assert st["fallback_pieces"] == 0
        _check_batched(ref, db, q, metric, k, got)

        h.set_tuning(100, 16)
        got = h.search_batched(q, k)
        st = _check_passes(h, n, 100, 16)
        assert st["fallback_pieces"] > 0
        _check_batched(ref, db, q, metric, k, got)

        for query in q[:2]:
            oi, od = one_to_many(oracle, db, query, metric, k)
            for tuning in ((0, 0), (100, 16)):
                h.set_tuning(*tuning)
                idx, dist, cnt = h.search(query, k)
                assert cnt == k
                np.testing.assert_array_equal(idx, oi)
                np.testing.assert_array_equal(_bits(dist), _bits(od))
    finally:
        h.close()
