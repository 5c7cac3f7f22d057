"""The search and build kernels past 128 dims, at K = 28 and at the exact
reorder's tails, against the oracle.

The other GPU tests stay at or below 128 dims and never build 53..56 blocks.
This file runs one small index per row of CASES through every stage, so that
the code which only these shapes reach runs under a test:

  * partition_scores_kernel<32> (dim > 128): 32-dim staging rounds, clamped
    loads, the padded last MFMA step and its own squared-L2 query norm;
  * the four branches of the rank kernel's 8-lane exact reorder (dims
    96..103, 128..135, other dims up to 128, and the generic loop) with each
    of their 4-, 2- and 1-wide tails, and dims below 8;
  * the scalar reorder of the block select kernel (k' > 256);
  * K = 28 (53..56 blocks) and K = 20 of the scan, seed and leaf-score
    kernels, in both tile widths, and the overflow rescan at K = 28 and 32;
  * the lookup table with 3, 4 and 12 dims per block and a partial last block;
  * the build kernels (assignment, plain and AVQ encoding) past 128 dims.

Every search comparison is equality of ids, counts and distance bits with
the oracle's ideal mode; tests/test_oracle_wide_dims.py pins
the oracle itself at these widths.  test_cases_reach_every_branch restates
the kernels' dispatch rules and fails if an edit of CASES drops a branch.
"""
import os

import numpy as np
import pytest

from tests.conftest import make_index

gpu = pytest.mark.gpu

DOT, L2 = 0, 1
# dim, dims per block, metric (a dot index from make_index is residual, with
# unit rows; squared L2 is non-residual on unnormalised rows)
CASES = [
    dict(d=129, dpb=3, metric=DOT),   # 43 blocks, K = 24; chunked partition, last chunk of 1
    dict(d=131, dpb=4, metric=L2),    # 33 blocks, K = 20; reorder tails 2 + 1; last block of 3
    dict(d=135, dpb=3, metric=L2),    # 45 blocks, K = 24; reorder tails 4 + 2 + 1
    dict(d=136, dpb=4, metric=DOT),   # 34 blocks, K = 20; first dim on the generic reorder loop
    dict(d=161, dpb=3, metric=DOT),   # 54 blocks, K = 28; five whole chunks + 1
    dict(d=200, dpb=4, metric=DOT),   # 50 blocks, K = 26 (dense-first tile); last chunk of 8
    dict(d=255, dpb=4, metric=L2),    # 64 blocks, K = 32; padded last MFMA step; last block of 3
    dict(d=256, dpb=4, metric=L2),    # 64 blocks, K = 32; whole chunks only
    dict(d=768, dpb=12, metric=DOT),  # 64 blocks of 12 dims, 24 chunks
    dict(d=110, dpb=2, metric=L2),    # 55 blocks, K = 28 on the full-dim partition kernel
    dict(d=97, dpb=2, metric=DOT),    # 49..52 blocks, K = 26: the dims 96..103 reorder
    dict(d=99, dpb=2, metric=L2),
    dict(d=101, dpb=2, metric=DOT),
    dict(d=103, dpb=2, metric=L2),
    dict(d=1, dpb=1, metric=L2),      # below 8 dims: the reorder is all tail
    dict(d=2, dpb=1, metric=L2),
    dict(d=3, dpb=2, metric=L2),
    dict(d=5, dpb=2, metric=L2),
    dict(d=7, dpb=3, metric=L2),
]
LEAVES = 70      # one full 64-center tile and one of 6
N_ROWS = 3000    # uneven leaves (1..250 rows): 9 of them hold from below to above k' = 300 rows


def _name(c):
    return f"{c['d']}x{c['dpb']}-{'dot' if c['metric'] == DOT else 'l2'}"


def _pick(**kw):
    got = [c for c in CASES if all(c[k] == v for k, v in kw.items())]
    assert got, kw
    return got


# ---- the kernels' dispatch rules, restated --------------------------------
def blocks_of(c):
    return -(-c["d"] // c["dpb"])


def ksteps_of(blocks):
    """EffectiveKSteps: the first compiled scan K >= ceil(blocks / 2)."""
    return next(k for k in (4, 8, 12, 16, 20, 24, 26, 28, 32) if k >= (blocks + 1) // 2)


def reorder_branch(dim):
    """ExactDistances8's choice by the whole 8-dim steps j8 = dim & ~7."""
    j8 = dim & ~7
    if j8 == 0:
        return "tail_only"
    if j8 == 96:
        return "exact12"
    if j8 == 128:
        return "exact16"
    return "clamped" if dim <= 128 else "generic"


def reorder_tails(dim):
    r = dim & 7
    return {w for w in (4, 2, 1) if r & w}


def last_chunk(dim):
    """Dims of the chunked partition kernel's last 32-dim round (dim > 128)."""
    return dim - 32 * ((dim - 1) // 32)


def test_cases_reach_every_branch():
    assert len({_name(c) for c in CASES}) == len(CASES)
    assert all(blocks_of(c) <= 64 for c in CASES)
    ks = {ksteps_of(blocks_of(c)) for c in CASES}
    assert {20, 26, 28, 32} <= ks
    assert {blocks_of(c) for c in CASES if ksteps_of(blocks_of(c)) == 28} == {54, 55}
    dims = [c["d"] for c in CASES]
    by_branch = {}
    for d in dims:
        by_branch.setdefault(reorder_branch(d), set()).update(reorder_tails(d))
    assert set(by_branch) == {"tail_only", "exact12", "exact16", "clamped", "generic"}
    assert by_branch["exact12"] == {4, 2, 1} and by_branch["exact16"] == {4, 2, 1}
    assert by_branch["tail_only"] == {4, 2, 1}
    # clamped loads with fewer steps than the 16 held in registers, past 64 dims
    assert any(reorder_branch(d) == "clamped" and 13 <= d // 8 <= 15 for d in dims)
    assert 136 in dims and any(reorder_branch(d) == "generic" and d % 8 for d in dims)
    wide = [d for d in dims if d > 128]
    lasts = {last_chunk(d) for d in wide}
    assert 1 in lasts and 32 in lasts and any(v % 2 and v > 1 for v in lasts)
    assert any(d <= 128 and ksteps_of(blocks_of(c)) == 28 for c, d in zip(CASES, dims))
    assert {c["metric"] for c in CASES if c["d"] > 128} == {DOT, L2}
    # dims per block above 4, and a partial last block of more than 2 dims past 128 dims
    assert any(c["dpb"] > 4 for c in CASES)
    assert any(c["d"] > 128 and c["dpb"] > 2 and 2 < c["d"] % c["dpb"] for c in CASES)


# ---- one index, one handle and one set of oracle results per case ---------
class _Built:
    def __init__(self, oracle, case, leaves=LEAVES):
        from scann_amd import _native
        self.oracle = oracle
        self.ix, self.db, self.q = make_index(n=N_ROWS, d=case["d"], leaves=leaves,
                                              dpb=case["dpb"], metric=case["metric"],
                                              seed=500 + case["d"], components=12)
        assert self.ix.num_blocks == blocks_of(case) and self.ix.dim == case["d"]
        assert self.ix.residual == (case["metric"] == DOT)
        self.nat = _native.NativeIndex(self.ix)
        self._ref = {}

    def search(self, L, pre, final, reorder):
        key = (L, pre, final, reorder)
        if key not in self._ref:
            o = self.oracle
            self._ref[key] = o.search(self.ix, self.q, L, pre, final, reorder, o.MODE_IDEAL)
        return self._ref[key]

    def pre_reorder(self, L, pre):
        key = (L, pre)
        if key not in self._ref:
            o = self.oracle
            self._ref[key] = o.search_pre_reorder(self.ix, self.q, L, pre, o.MODE_IDEAL)
        return self._ref[key]


@pytest.fixture(scope="module")
def built(oracle):
    cache = {}

    def get(case):
        if _name(case) not in cache:
            cache[_name(case)] = _Built(oracle, case)
        return cache[_name(case)]

    yield get
    for b in cache.values():
        b.nat.close()


def _handle(ix, env):
    from scann_amd import _native
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return _native.NativeIndex(ix)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(got, want, tag):
    (gi, gd, gc), (oi, od, oc) = got, want
    np.testing.assert_array_equal(gc, oc, err_msg=tag)
    np.testing.assert_array_equal(gi, oi, err_msg=tag)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32), err_msg=tag)


all_cases = pytest.mark.parametrize("case", CASES, ids=_name)


def _check_partition(oracle, b, tag):
    """Every score of the row (L = num_leaves) and the best one (L = 1), at
    1, 63, 64 and 65 queries: the 65th is a perturbed copy of the first, alone
    in a second query tile whose other 63 rows clamp to it."""
    ix, q = b.ix, b.q
    rng = np.random.default_rng(ix.dim)
    extra = q[:1] + np.float32(1e-3) * rng.standard_normal((1, ix.dim)).astype(np.float32)
    q65 = np.concatenate([q, extra]).astype(np.float32)
    for L in (ix.num_leaves, 1):
        ol, od = oracle.partition_topl(q65, ix.centers, ix.metric, L)
        for nq in (1, 63, 64, 65):
            gl, gd = b.nat.partition_topl(q65[:nq], L)
            np.testing.assert_array_equal(gl, ol[:nq], err_msg=f"{tag} nq={nq} L={L}")
            np.testing.assert_array_equal(gd.view(np.uint32), od[:nq].view(np.uint32),
                                          err_msg=f"{tag} nq={nq} L={L}")


@gpu
@all_cases
def test_partition_scores_of_every_leaf(oracle, built, case):
    _check_partition(oracle, built(case), _name(case))


@gpu
def test_partition_scores_three_center_tiles(oracle):
    """130 leaves at 161 dims: center tiles of 64, 64 and 2."""
    case = _pick(d=161)[0]
    b = _Built(oracle, case, leaves=130)
    try:
        assert b.ix.num_leaves == 130
        _check_partition(oracle, b, "161 dims, 130 leaves")
    finally:
        b.nat.close()


@gpu
@all_cases
def test_lookup_tables(oracle, built, case):
    b = built(case)
    lut, mult = b.nat.create_lookup_tables(b.q)
    for i in range(b.q.shape[0]):
        _, u8, m = oracle.create_lut(b.q[i], b.ix.codebook, b.ix.metric)
        np.testing.assert_array_equal(lut[i], u8, err_msg=f"{_name(case)} query {i}")
        assert np.float32(m).view(np.uint32) == mult[i].view(np.uint32), (_name(case), i)


@gpu
@all_cases
def test_exact_distances(oracle, built, case):
    b = built(case)
    rng = np.random.default_rng(case["d"])
    ids = rng.integers(0, b.ix.num_datapoints, (b.q.shape[0], 5)).astype(np.uint32)
    got = b.nat.exact_distances(b.q, ids)
    want = np.array([[oracle.exact_distance(b.q[i], b.db[ids[i, j]], b.ix.metric)
                      for j in range(ids.shape[1])] for i in range(ids.shape[0])], np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@gpu
@pytest.mark.parametrize("pre", [100, 300])
@all_cases
def test_batched_search(built, case, pre):
    """k' = 100 ends in the rank kernel and its 8-lane reorder, k' = 300 in
    the block select kernel and the scalar reorder."""
    b = built(case)
    L, final = 9, 10
    tag = f"{_name(case)} pre={pre}"
    _same(b.nat.search_pre_reorder(b.q, L, pre), b.pre_reorder(L, pre), tag)
    for reorder in (True, False):
        got = b.nat.search_batched(b.q, L, pre, final, reorder)
        assert (got[2] == final).all(), tag
        _same(got, b.search(L, pre, final, reorder), f"{tag} reorder={reorder}")


@gpu
@pytest.mark.parametrize("reorder", [True, False])
@all_cases
def test_single_query_search(oracle, built, case, reorder):
    """search() scores the leaves in the one-to-many (A.8) order."""
    b = built(case)
    mode = oracle.MODE_IDEAL | oracle.PARTITION_ONE_TO_MANY
    for i in range(6):
        gi, gd, gc = b.nat.search(b.q[i], 9, 100, 10, reorder)
        oi, od, oc = oracle.search(b.ix, b.q[i:i + 1], 9, 100, 10, reorder, mode)
        assert gc == int(oc[0]) == 10
        np.testing.assert_array_equal(gi[:gc], oi[0, :gc])
        np.testing.assert_array_equal(gd[:gc].view(np.uint32), od[0, :gc].view(np.uint32))


K28 = [c for c in CASES if ksteps_of(blocks_of(c)) == 28]
K20 = [c for c in CASES if ksteps_of(blocks_of(c)) == 20]


@gpu
@pytest.mark.parametrize("case", K28 + K20, ids=_name)
def test_leaf_scores(oracle, built, case):
    b = built(case)
    ix = b.ix
    sizes = np.diff(ix.leaf_offsets.astype(np.int64))
    filled = np.flatnonzero(sizes > 0)
    leaves = {int(filled[sizes[filled].argmin()]), int(sizes.argmax()), 0, ix.num_leaves - 1}
    lut, _ = b.nat.create_lookup_tables(b.q[:2])
    for leaf in sorted(leaves):
        lo, hi = int(ix.leaf_offsets[leaf]), int(ix.leaf_offsets[leaf + 1])
        if hi == lo:
            continue
        packed = oracle.pack_codes(ix.member_codes[lo:hi])
        for qi in range(2):
            want = oracle.lut16_accumulate(packed, hi - lo, ix.num_blocks, lut[qi])
            np.testing.assert_array_equal(b.nat.leaf_scores(leaf, lut[qi]), want,
                                          err_msg=f"{_name(case)} leaf {leaf}")


def _tile_paths(case):
    paths = [{"SMX_NARROW": "0"}, {"SMX_NARROW": "2"}]
    if ksteps_of(blocks_of(case)) % 4 == 2:   # the dense-first 32-slot tile and the all-sparse one
        paths = [{"SMX_NARROW": "0", "SMX_DENSE_FIRST": "1"},
                 {"SMX_NARROW": "0", "SMX_DENSE_FIRST": "0"}, {"SMX_NARROW": "2"}]
    return paths


@gpu
@pytest.mark.parametrize("case", K28 + _pick(d=200), ids=_name)
def test_tile_widths(built, case):
    """32-slot tiles only and 16-slot tiles only: the oracle's results, and the
    same candidates under the same thresholds."""
    b = built(case)
    want = b.search(9, 100, 10, True)
    cands = set()
    for env in _tile_paths(case):
        nat = _handle(b.ix, env)
        try:
            nat.set_profiling(True)
            got = nat.search_batched(b.q, 9, 100, 10, True)
            cands.add(nat.timings()["mean_candidates"])
        finally:
            nat.close()
        _same(got, want, f"{_name(case)} {env}")
    assert len(cands) == 1, cands


@gpu
@pytest.mark.parametrize("case", K28 + _pick(d=256), ids=_name)
def test_overflow_rescan(built, case):
    """A 600-key list, no seed threshold and every leaf searched: every list
    overflows, and the block select kernel rescans it on the device."""
    from scann_amd import _native
    b = built(case)
    nat = _native.NativeIndex(b.ix)
    try:
        nat.set_tuning(600, 0, 0, 32)
        nat.set_profiling(True)
        got = nat.search_pre_reorder(b.q, LEAVES, 300)
        assert nat.timings()["overflow_retries"] >= 1
    finally:
        nat.close()
    assert (got[2] == 300).all()
    _same(got, b.pre_reorder(LEAVES, 300), _name(case))


@gpu
@pytest.mark.parametrize("case", _pick(d=161) + _pick(d=256), ids=_name)
def test_two_shards_with_their_own_rows(built, case):
    import torch
    from scann_amd.distributed import NativeShardEngine
    b = built(case)
    L, pre, final, world = 9, 100, 10, 2
    engines = [NativeShardEngine(b.ix.shard(r, world, own_rows=True), device=0)
               for r in range(world)]
    try:
        qd = torch.from_numpy(b.q).cuda()
        nq = b.q.shape[0]
        k = engines[0].shard_width(L, pre, final, True)
        entries = torch.empty((world, nq, k, 2), dtype=torch.int64, device="cuda")
        for r, e in enumerate(engines):
            e.search_shard(qd, L, pre, final, True, entries[r])
        idx, dst, cnt = engines[0].merge(world, entries, nq, L, pre, final, True)
        torch.cuda.synchronize()
        got = (idx.cpu().numpy().astype(np.uint32), dst.cpu().numpy(), cnt.cpu().numpy())
    finally:
        for e in engines:
            e.nat.close()
    _same(got, b.search(L, pre, final, True), _name(case))


# ---- the build kernels past 128 dims --------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@gpu
@pytest.mark.parametrize("n,dim,dpb,thr", [(300, 131, 4, 0.2), (200, 200, 4, 0.3)])
def test_avq_encode_wide(oracle, n, dim, dpb, thr):
    from scann_amd import device_builder as db
    rng = np.random.default_rng(dim * 7 + n)
    nb = -(-dim // dpb)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    c = rng.standard_normal((8, dim)).astype(np.float32) * 0.3
    r = (x - c[rng.integers(0, 8, n)]).astype(np.float32)
    cb = (rng.standard_normal((nb, 16, dpb)) * 0.2).astype(np.float32)
    got = db.avq_encode(_dev(r), _dev(x), _dev(cb), thr).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.avq_encode(r, x, cb, thr))


def _block_encode_ref(r, cb):
    """Squared L2 to each of a block's 16 centers, summed in coordinate order
    in float32 (the last block zero-padded), first minimum."""
    n, dim = r.shape
    nb, _, dpb = cb.shape
    pad = np.zeros((n, nb * dpb), np.float32)
    pad[:, :dim] = r
    v = pad.reshape(n, nb, 1, dpb) - cb[None]
    d = np.zeros((n, nb, 16), np.float32)
    for i in range(dpb):
        d = (d + v[..., i] * v[..., i]).astype(np.float32)
    return d.argmin(-1).astype(np.uint8)


@gpu
def test_block_encode_wide():
    from scann_amd import device_builder as db
    n, dim, dpb = 500, 255, 4
    rng = np.random.default_rng(n + dim)
    nb = -(-dim // dpb)
    r = rng.standard_normal((n, dim)).astype(np.float32)
    cb = rng.standard_normal((nb, 16, dpb)).astype(np.float32)
    got = db.block_encode(_dev(r), _dev(cb)).cpu().numpy()
    np.testing.assert_array_equal(got, _block_encode_ref(r, cb))


def _nearest(x, c, primary=None, lam=0.0):
    import torch
    from scann_amd import _native
    xd, cd = _dev(x), _dev(c)
    out = torch.empty(x.shape[0], dtype=torch.int32, device="cuda")
    pd = None if primary is None else _dev(primary.astype(np.int32))
    _native.nearest_centers_device(xd.data_ptr(), x.shape[0], x.shape[1], cd.data_ptr(),
                                   c.shape[0], out.data_ptr(),
                                   None if pd is None else pd.data_ptr(), lam)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_nearest(got, loss64):
    """The kernel computes in float32: rows whose two best float64 losses are
    within a relative 1e-4 may differ, every other row must match (the rule
    of tests/test_gpu_builder.py)."""
    order = np.argsort(loss64, axis=1, kind="stable")
    best = order[:, 0]
    b0 = loss64[np.arange(len(best)), best]
    b1 = loss64[np.arange(len(best)), order[:, 1]]
    clear = (b1 - b0) > 1e-4 * np.maximum(1.0, np.abs(b0))
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(got[clear], best[clear])


@gpu
@pytest.mark.parametrize("soar", [False, True])
def test_nearest_centers_wide(soar):
    """161 dims: five whole 32-dim staging rounds and one of a single dim; 130
    centers: center tiles of 64, 64 and 2."""
    n, d, k, lam = 1000, 161, 130, 1.5
    rng = np.random.default_rng(n + d + k)
    c = rng.standard_normal((k, d)).astype(np.float32)
    x = (c[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    diff = x64[:, None, :] - c64[None]
    loss = (diff ** 2).sum(-1)
    if not soar:
        _check_nearest(_nearest(x, c), loss)
        return
    primary = loss.argmin(1)
    got = _nearest(x, c, primary, lam)
    assert not np.any(got == primary)
    r = x64 - c64[primary]
    loss = loss + lam * (np.einsum("nd,nkd->nk", r, diff) ** 2) / \
        np.maximum((r * r).sum(1), 1e-30)[:, None]
    loss[np.arange(n), primary] = np.inf
    _check_nearest(got, loss)


@gpu
def test_device_built_index_wide(oracle):
    """An index built on the device at 136 dims, 4 per block, searches like
    the oracle on that index."""
    from scann_amd import _native, synthetic
    from scann_amd import device_builder as db
    x = synthetic.mixture(4000, 136, 32, 0.9, seed=13)
    q = synthetic.mixture(48, 136, 32, 0.9, seed=113, means_seed=13)
    ix = db.build_tree_ah(x, DOT, 32, 4, training_iterations=6, ah_training_iterations=6, seed=3)
    assert ix.num_blocks == 34 and ix.num_leaves == 32 and ix.num_members == 4000
    nat = _native.NativeIndex(ix)
    try:
        got = nat.search_batched(q, 8, 100, 10, True)
        pre = nat.search_pre_reorder(q, 8, 100)
    finally:
        nat.close()
    assert (got[2] == 10).all()
    _same(got, oracle.search(ix, q, 8, 100, 10, True, oracle.MODE_IDEAL), "search")
    _same(pre, oracle.search_pre_reorder(ix, q, 8, 100, oracle.MODE_IDEAL), "pre-reorder")
