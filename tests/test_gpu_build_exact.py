"""The index-build kernels (scann_amd/csrc/smx_builder.hip, smx_sort.hip) and
their driver (scann_amd/device_builder.py) against the exact references of
tests/build_ref.py, at the shapes where they can go wrong:

1. smx_nearest_centers, k-means and SOAR: every row within a derived float32
   error bound of the float64 argmin (and equal to it wherever the bound
   leaves no second candidate), the returned loss within the bound, exact
   ties to the lowest index across strips and tiles, SOAR rows with a zero
   residual; n around the 64-row block, k around the 64-center tile, d
   around the 32-dimension chunk;
2. the fixed-point mean step (smx_kmeans_accumulate, smx_codebook_accumulate,
   smx_kmeans_finalize): sums, counts and centers bit for bit, on both sides
   of the LDS / global switch of the codebook accumulation;
3. smx_group_by_leaf, smx_gather_residuals, smx_block_encode, smx_avq_encode
   at their edges;
4. device_builder.kmeans, train_codebook and build_tree_ah: the produced
   centers, codebook and index themselves.

Every dataset's CPU-side precondition (few ambiguous rows, a tie that decides
the result, ...) is asserted before the GPU is touched, and again by the
unmarked tests at the end of the file.
"""
import numpy as np
import pytest

from tests import build_ref as R

gpu = pytest.mark.gpu
LAM = 1.5


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# 1. nearest center and SOAR
# ---------------------------------------------------------------------------
def _nearest(x, c, primary=None, lam=0.0):
    import torch
    from scann_amd import _native
    xd, cd = _dev(x), _dev(c)
    n = x.shape[0]
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    pd = None if primary is None else _dev(primary.astype(np.int32))
    _native.nearest_centers_device(xd.data_ptr(), n, x.shape[1], cd.data_ptr(), c.shape[0],
                                   out.data_ptr(), None if pd is None else pd.data_ptr(), lam,
                                   loss.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy()


def _assign_case(family, n, k, d, soar):
    """(x, c, primary, LOSS, B) of one case, its 2 % condition asserted."""
    spread = R.SOAR_OFFSET_SPREAD if soar and family == "offset" else 1.0
    x, c = R.assignment_dataset(family, n, k, d, R.case_seed(family, n, k, d), spread)
    if soar:
        primary = R.primary_of(x, c)
        loss, bound = R.soar_loss_bound(x, c, primary, LAM)
    else:
        primary = None
        loss, bound = R.kmeans_loss_bound(x, c)
    _, amb = R.ambiguous_rows(loss, bound)
    assert amb.sum() <= 0.02 * n, f"{amb.sum()} of {n} rows ambiguous"
    return x, c, primary, loss, bound


_IDS = [f"{f}-n{n}-k{k}-d{d}" for f, n, k, d in R.ASSIGN_CASES]


@gpu
@pytest.mark.parametrize("family,n,k,d", R.ASSIGN_CASES, ids=_IDS)
def test_kmeans_assignment_every_row(family, n, k, d):
    x, c, _, loss, bound = _assign_case(family, n, k, d, False)
    got, got_loss = _nearest(x, c)
    R.check_assignment(got, got_loss, loss, bound)


_SOAR_CASES = [t for t in R.ASSIGN_CASES if t[2] >= 2]


@gpu
@pytest.mark.parametrize("family,n,k,d", _SOAR_CASES,
                         ids=[i for i, t in zip(_IDS, R.ASSIGN_CASES) if t[2] >= 2])
def test_soar_assignment_every_row(family, n, k, d):
    x, c, primary, loss, bound = _assign_case(family, n, k, d, True)
    got, got_loss = _nearest(x, c, primary, LAM)
    assert not np.any(got == primary)
    R.check_assignment(got, got_loss, loss, bound)


# duplicated centers (low, high): one thread's 4-center strip; two strips of
# one 64-center tile; one thread's strip in two tiles; two threads in two tiles
TIE_PAIRS = [(8, 10), (5, 41), (20, 84), (50, 129)]
TIE_PRIMARY = 3


def _tie_case(soar):
    """130 centers with the four duplicated pairs and 70 rows (two row
    blocks), each nearest to a duplicated center; CPU precondition: the pair
    is the float64 best and nothing else is inside the bound of it."""
    rng = np.random.default_rng(77)
    k, d, n = 130, 33, 70
    c = (4.0 * rng.standard_normal((k, d))).astype(np.float32)
    for lo, hi in TIE_PAIRS:
        c[hi] = c[lo]
    which = np.arange(n) % len(TIE_PAIRS)
    lows = np.array([p[0] for p in TIE_PAIRS])[which]
    highs = np.array([p[1] for p in TIE_PAIRS])[which]
    x = (c[lows] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    if soar:
        primary = np.full(n, TIE_PRIMARY, np.int32)
        loss, bound = R.soar_loss_bound(x, c, primary, LAM)
    else:
        primary = None
        loss, bound = R.kmeans_loss_bound(x, c)
    rows = np.arange(n)
    np.testing.assert_array_equal(loss.argmin(1), lows)       # first minimum: the lower copy
    np.testing.assert_array_equal(loss[rows, lows], loss[rows, highs])
    lim = (loss[rows, lows] + bound[rows, lows])[:, None] + bound
    within = loss <= lim
    assert np.all(within.sum(1) == 2)                         # the two copies and nothing else
    return x, c, primary, lows


@gpu
@pytest.mark.parametrize("soar", [False, True], ids=["kmeans", "soar"])
def test_assignment_ties_go_to_the_lowest_index(soar):
    x, c, primary, lows = _tie_case(soar)
    got, _ = _nearest(x, c, primary, LAM if soar else 0.0)
    np.testing.assert_array_equal(got, lows)


def _zero_residual_case():
    x, c = R.assignment_dataset("blobs", 65, 65, 33, 4242)
    primary = R.primary_of(x, c)
    x[::3] = c[primary[::3]]                  # bit for bit their primary center
    primary = R.primary_of(x, c)
    assert np.all((x[::3] == c[primary[::3]]).all(1))
    loss, bound = R.soar_loss_bound(x, c, primary, LAM)
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    plain = ((x64[::3, None, :] - c64[None]) ** 2).sum(-1)
    plain[np.arange(plain.shape[0]), primary[::3]] = np.inf
    np.testing.assert_array_equal(loss[::3], plain)           # the penalty term is exactly 0
    _, amb = R.ambiguous_rows(loss, bound)
    assert amb.sum() <= 0.02 * x.shape[0]
    return x, c, primary, loss, bound


@gpu
def test_soar_zero_residual_rows():
    x, c, primary, loss, bound = _zero_residual_case()
    got, got_loss = _nearest(x, c, primary, LAM)
    assert not np.any(got == primary)
    assert np.all(np.isfinite(got_loss))
    R.check_assignment(got, got_loss, loss, bound)


# ---------------------------------------------------------------------------
# 2. fixed-point mean steps, bit for bit
# ---------------------------------------------------------------------------
SENTINEL = 7.0


def _finalize(sums, cnt, k, d, scale):
    import torch
    from scann_amd import _native
    from scann_amd import device_builder as db
    cen = torch.full((k, d), SENTINEL, dtype=torch.float32, device="cuda")
    _native.check(_native.load().smx_kmeans_finalize(db._p(sums), db._p(cnt), k, d, scale,
                                                     db._p(cen), None), "fin")
    torch.cuda.synchronize()
    return cen.cpu().numpy()


def _kmeans_mean_step(x, lab, k, scale):
    import torch
    from scann_amd import _native
    from scann_amd import device_builder as db
    n, d = x.shape
    xd, ld = _dev(x), _dev(lab.astype(np.int32))
    sums = torch.zeros(k * d, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(k, dtype=torch.int32, device="cuda")
    _native.check(_native.load().smx_kmeans_accumulate(db._p(xd), n, d, db._p(ld), k, scale,
                                                       db._p(sums), db._p(cnt), None), "acc")
    cen = _finalize(sums, cnt, k, d, scale)
    return sums.cpu().numpy().reshape(k, d), cnt.cpu().numpy().astype(np.int64), cen


def _mean_case(name):
    """(x, labels, k, scale).  Labels -1 and k contribute nothing; one center
    of [0, k) gets no row."""
    from scann_amd.device_builder import fixed_point_scale
    rng = np.random.default_rng(len(name) + 11)
    if name == "half":          # x * scale ends in .5: llrint's half-to-even, not truncation
        n, d, k = 1000, 1, 3
        scale = 1024.0
        x = ((rng.integers(-2000, 2000, (n, d)) + 0.5) / scale).astype(np.float32)
        lab = rng.choice([-1, 0, 2, 3], n)                    # center 1 empty
    elif name in ("oob", "scale1000"):
        n, d, k = 257, 7, 5
        x = (3.0 * rng.standard_normal((n, d))).astype(np.float32)
        lab = rng.choice([-1, 0, 1, 3, 4, 5], n)              # center 2 empty
        # any positive scale is accepted; with 1000, no power of two, x * scale
        # is itself rounded and the division by the scale is inexact
        scale = 1000.0 if name == "scale1000" else fixed_point_scale(float(np.abs(x).max()), n)
    elif name == "random":
        n, d, k = 4096, 24, 37
        x = (3.0 * rng.standard_normal((n, d))).astype(np.float32)
        lab = rng.integers(-1, k + 1, n)
        lab[lab == 36] = 35                                   # center 36 empty
        scale = fixed_point_scale(float(np.abs(x).max()), n)
    else:                       # "top": one center takes every row, values +-max_abs
        n, d, k = 4096, 24, 37
        x = np.where(np.arange(d) % 2 == 0, 3.75, -3.75).astype(np.float32)[None].repeat(n, 0)
        lab = np.full(n, 17)
        scale = fixed_point_scale(3.75, n)
        assert n * 3.75 * scale > 2.0 ** 60                   # the top of the allowed range
    return np.ascontiguousarray(x), lab.astype(np.int32), k, scale


MEAN_CASES = ["half", "oob", "scale1000", "random", "top"]


@gpu
@pytest.mark.parametrize("name", MEAN_CASES)
def test_kmeans_mean_step_bits(name):
    x, lab, k, scale = _mean_case(name)
    want_s, want_c = R.fixed_sums(x, lab, k, scale)
    assert (want_c == 0).any() and (want_c > 0).any()
    if name == "half":
        frac = np.abs(x.astype(np.float64) * scale) % 1.0
        assert np.all(frac == 0.5)
    sums, cnt, cen = _kmeans_mean_step(x, lab, k, scale)
    np.testing.assert_array_equal(cnt, want_c)
    np.testing.assert_array_equal(sums, want_s)
    want = R.fixed_means(want_s, want_c, scale, np.full((k, x.shape[1]), SENTINEL, np.float32))
    np.testing.assert_array_equal(cen.view(np.uint32), want.view(np.uint32))
    assert np.all(cen[want_c == 0] == SENTINEL)               # empty centers keep their value


def _codebook_step(r, codes, nb, dpb, scale):
    import torch
    from scann_amd import _native
    from scann_amd import device_builder as db
    n, dim = r.shape
    rd, cd = _dev(r), _dev(codes)
    sums = torch.zeros(nb * 16 * dpb, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(nb * 16, dtype=torch.int32, device="cuda")
    _native.check(_native.load().smx_codebook_accumulate(db._p(rd), n, dim, db._p(cd), nb, dpb,
                                                         scale, db._p(sums), db._p(cnt), None),
                  "acc")
    cen = _finalize(sums, cnt, nb * 16, dpb, scale)
    return sums.cpu().numpy().reshape(nb * 16, dpb), cnt.cpu().numpy().astype(np.int64), cen


def codebook_lds_bytes(nb, dpb):
    return nb * 16 * dpb * 8 + nb * 16 * 4


# dim, dpb: 204 blocks in LDS (65 280 bytes, the largest at dpb 2), the same
# with a zero-padded last block, 205 blocks through global memory; dpb 1 on
# both sides of its switch (341 blocks: 65 472 bytes)
CODEBOOK_SHAPES = [(408, 2), (407, 2), (410, 2), (341, 1), (342, 1)]


@gpu
@pytest.mark.parametrize("half", [False, True], ids=["wide-scale", "half-integers"])
@pytest.mark.parametrize("n", [3000, 1])
@pytest.mark.parametrize("dim,dpb", CODEBOOK_SHAPES)
def test_codebook_mean_step_bits(dim, dpb, n, half):
    from scann_amd.device_builder import fixed_point_scale
    nb = -(-dim // dpb)
    lds = codebook_lds_bytes(nb, dpb)
    assert (lds <= 65536) == ((dim, dpb) in [(408, 2), (407, 2), (341, 1)])
    if n == 3000:
        assert n * nb > 2048 * 256                            # the LDS kernel's grid-stride loop wraps
    rng = np.random.default_rng(dim * 3 + n)
    if half:
        scale = 1024.0
        r = ((rng.integers(-2000, 2000, (n, dim)) + 0.5) / scale).astype(np.float32)
    else:
        r = rng.standard_normal((n, dim)).astype(np.float32)
        scale = fixed_point_scale(float(np.abs(r).max()), n)
    codes = rng.integers(0, 16, (n, nb)).astype(np.uint8)
    codes[:, 0] = 0 if n == 1 else codes[:, 0] % 3            # block 0, center 0 is used
    codes[0, 0] = 0
    want_s, want_c = R.codebook_sums(r, codes, nb, dpb, scale)
    sums, cnt, cen = _codebook_step(r, codes, nb, dpb, scale)
    np.testing.assert_array_equal(cnt, want_c)
    np.testing.assert_array_equal(sums, want_s)
    want = R.fixed_means(want_s, want_c, scale, np.full((nb * 16, dpb), SENTINEL, np.float32))
    np.testing.assert_array_equal(cen.view(np.uint32), want.view(np.uint32))
    if dim % dpb:
        assert np.all(sums[(nb - 1) * 16:, dpb - 1] == 0)     # the padded coordinate


# ---------------------------------------------------------------------------
# 3. group, gather, encode
# ---------------------------------------------------------------------------
def _group_case(k, m, layout):
    rng = np.random.default_rng(k * 1000 + m)
    ids = rng.permutation(m).astype(np.uint32)
    if layout == "random":
        lab = rng.integers(0, k, m)
    elif layout == "leaf0":
        lab = np.zeros(m, np.int64)
    elif layout == "last":
        lab = np.full(m, k - 1)
    elif layout == "topbit":            # ids >= 2^31: uint32 in int32 storage
        lab = rng.integers(0, k, m)
        ids = (ids * np.uint32(16777259) + np.uint32(0x7FFFFF00)).astype(np.uint32)
        assert (ids >= 2 ** 31).any() and (ids < 2 ** 31).any() and np.unique(ids).size == m
    else:                               # "soar": every id twice, in two different leaves
        h = m // 2
        first = rng.integers(0, k, h)
        second = (first + rng.integers(1, k, h)) % k
        lab = np.concatenate([first, second])
        ids = np.concatenate([np.arange(h), np.arange(h)]).astype(np.uint32)
    return lab.astype(np.int32), ids


_GROUP_CASES = [(k, m, "random") for k in (1, 2, 3, 4, 5, 1024, 1025) for m in (255, 256, 257)]
_GROUP_CASES += [(k, 257, lay) for k in (1, 5, 1025) for lay in ("leaf0", "last", "topbit")]
_GROUP_CASES += [(k, 256, "soar") for k in (2, 5, 1025)]


@gpu
@pytest.mark.parametrize("k,m,layout", _GROUP_CASES)
def test_group_by_leaf_edges(k, m, layout):
    from scann_amd import device_builder as db
    lab, ids = _group_case(k, m, layout)
    m = lab.size
    off, mem, ml = db.group_by_leaf(_dev(lab), _dev(ids.view(np.int32)), k)
    want_off, want_mem, want_ml = R.group_by_leaf(lab, ids, k)
    np.testing.assert_array_equal(mem.cpu().numpy().view(np.uint32), want_mem)
    np.testing.assert_array_equal(ml.cpu().numpy(), want_ml)
    np.testing.assert_array_equal(off.cpu().numpy(), want_off)


@gpu
@pytest.mark.parametrize("with_centers", [True, False], ids=["residual", "rows"])
@pytest.mark.parametrize("row_base", [0, 1000])
@pytest.mark.parametrize("d", [1, 3, 64])
def test_gather_residuals_bits(d, row_base, with_centers):
    from scann_amd import device_builder as db
    rng = np.random.default_rng(d + row_base)
    nloc, m, k = 20, 37, 6
    assert (m * d) % 256 != 0
    x = rng.standard_normal((nloc, d)).astype(np.float32)     # the local slice only
    c = rng.standard_normal((k, d)).astype(np.float32)
    local = rng.integers(0, nloc, m)                          # repeated rows
    local[:2] = [nloc - 1, 0]
    assert np.unique(local).size < m
    leaf = rng.integers(0, k, m).astype(np.int32)
    leaf[:2] = [k - 1, 0]
    rows = (local + row_base).astype(np.uint32)
    got = db.gather_residuals(_dev(x), _dev(rows.view(np.int32)), _dev(leaf),
                              _dev(c) if with_centers else None, row_base=row_base).cpu().numpy()
    want = (x[local] - c[leaf]).astype(np.float32) if with_centers else x[local]
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _block_encode_case(n, dim, dpb):
    """Rows and a codebook with duplicated centers (2 == 7 == 12 in every
    block), every third row exactly a duplicated center in every block."""
    rng = np.random.default_rng(n + dim + dpb)
    nb = -(-dim // dpb)
    cb = rng.standard_normal((nb, 16, dpb)).astype(np.float32)
    cb[:, 7] = cb[:, 2]
    cb[:, 12] = cb[:, 2]
    r = rng.standard_normal((n, dim)).astype(np.float32)
    r[::3] = cb[:, 2].reshape(-1)[:dim]
    return r, cb, nb


@gpu
@pytest.mark.parametrize("n,dim,dpb", [(85, 6, 2), (257, 1, 2), (51, 5, 1), (257, 1, 1),
                                       (85, 5, 2)])
def test_block_encode_edges(n, dim, dpb):
    from scann_amd import device_builder as db
    r, cb, nb = _block_encode_case(n, dim, dpb)
    assert n * nb in (255, 257)
    want = R.block_encode(r, cb)
    assert not np.isin(want, (7, 12)).any()                   # ties went to the lowest copy
    if dim % dpb == 0:
        assert np.all(want[::3] == 2)                         # the rows equal to center 2
    got = db.block_encode(_dev(r), _dev(cb)).cpu().numpy()
    np.testing.assert_array_equal(got, want)


AVQ_THR = 0.2


def _avq_case(n, dim, dpb, seed=0):
    """Residuals, datapoints and a codebook with: two identical blocks (1 and
    4) holding the same residual and datapoint values (equal residual norms:
    the block-order tie), duplicated centers inside block 2, and, from two
    rows up, a last datapoint row of all zeros (||x||^2 = 0: infinite and NaN
    arithmetic that both sides must resolve the same way)."""
    rng = np.random.default_rng(1000 * seed + dim * 7 + n)
    nb = -(-dim // dpb)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    c = rng.standard_normal((8, dim)).astype(np.float32) * 0.3
    r = (x - c[rng.integers(0, 8, n)]).astype(np.float32)
    cb = (rng.standard_normal((nb, 16, dpb)) * 0.2).astype(np.float32)
    cb[4] = cb[1]
    cb[2, 9] = cb[2, 3]
    for a in (r, x):
        a[:, 4 * dpb:5 * dpb] = a[:, dpb:2 * dpb]
    if n >= 2:
        x[n - 1] = 0.0
    return r, x, cb


@gpu
@pytest.mark.parametrize("dim,dpb", [(17, 2), (31, 3)])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_avq_encode_partial_blocks_and_ties(oracle, n, dim, dpb):
    from scann_amd import device_builder as db
    r, x, cb = _avq_case(n, dim, dpb)
    want = oracle.avq_encode(r, x, cb, AVQ_THR)
    got = db.avq_encode(_dev(r), _dev(x), _dev(cb), AVQ_THR).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    if n >= 2:      # the zero row: no move is ever accepted, the plain codes remain
        np.testing.assert_array_equal(want[n - 1], R.block_encode(r[n - 1:], cb)[0])


# (n, dim, dpb, seed, threshold) of two datasets, their property shown on the
# CPU by the Python restatement of the oracle: one whose block-order tie
# decides the codes, one whose rows change codes in a second round
AVQ_TIE_CASE = (7, 17, 2, 1, 0.5)
AVQ_ROUNDS_CASE = (7, 31, 3, 3, 0.7)


def _avq_special_case(oracle, case):
    n, dim, dpb, seed, thr = case
    r, x, cb = _avq_case(n, dim, dpb, seed=seed)
    want = oracle.avq_encode(r, x, cb, thr)
    fwd, rounds = R.avq_encode_py(r, x, cb, thr)
    np.testing.assert_array_equal(fwd, want)                  # the restatement is the oracle
    if case == AVQ_TIE_CASE:
        rev, _ = R.avq_encode_py(r, x, cb, thr, reverse_ties=True)
        assert (rev != want).any()                            # the tie's order decides codes
    else:
        one, _ = R.avq_encode_py(r, x, cb, thr, max_rounds=1)
        assert rounds.max() >= 2 and (one != want).any()      # a second round changes codes
    return r, x, cb, thr, want


@gpu
@pytest.mark.parametrize("case", [AVQ_TIE_CASE, AVQ_ROUNDS_CASE], ids=["order-tie", "rounds"])
def test_avq_block_order_tie_and_rounds(oracle, case):
    from scann_amd import device_builder as db
    r, x, cb, thr, want = _avq_special_case(oracle, case)
    got = db.avq_encode(_dev(r), _dev(x), _dev(cb), thr).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------
# 4. the driver
# ---------------------------------------------------------------------------
def _blobs(n, d, k, seed, spread=6.0, noise=0.3):
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((k, d))
    return (means[rng.integers(0, k, n)] + noise * rng.standard_normal((n, d))).astype(np.float32)


def _lloyd_step_ref(x, centers, rng):
    """One step of device_builder.kmeans on the host: float64 argmin (asserted
    unambiguous), the fixed-point means, empty centers re-seeded."""
    from scann_amd.device_builder import fixed_point_scale
    n, k = x.shape[0], centers.shape[0]
    loss, bound = R.kmeans_loss_bound(x, centers)
    best, amb = R.ambiguous_rows(loss, bound)
    assert not amb.any()
    scale = fixed_point_scale(float(np.abs(x).max()), n)
    s, cnt = R.fixed_sums(x, best.astype(np.int32), k, scale)
    out = R.fixed_means(s, cnt, scale, centers)
    empty = np.flatnonzero(cnt == 0)
    if empty.size:
        out[empty] = x[rng.choice(n, empty.size, replace=False)]
    return out


def _kmeans_one_step_case():
    x = _blobs(1500, 9, 12, seed=31)
    seed, k = 5, 12
    rng = np.random.default_rng(seed)
    init = x[rng.choice(x.shape[0], k, replace=False)]
    return x, k, seed, _lloyd_step_ref(x, init, rng)


@gpu
def test_kmeans_one_iteration_is_the_reference_step():
    from scann_amd import device_builder as db
    x, k, seed, want = _kmeans_one_step_case()
    got = db.kmeans(_dev(x), k, 1, seed).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@gpu
def test_kmeans_same_seed_same_bits():
    from scann_amd import device_builder as db
    x = _blobs(3000, 16, 24, seed=8, spread=1.0, noise=1.0)   # overlapping: real Lloyd steps
    xd = _dev(x)
    a = db.kmeans(xd, 24, 6, 3).cpu().numpy()
    b = db.kmeans(xd, 24, 6, 3).cpu().numpy()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(np.isfinite(a))


@gpu
@pytest.mark.parametrize("n,k", [(5, 5), (5, 8), (1, 3)])
def test_kmeans_k_at_least_n_returns_rows_then_zeros(n, k):
    from scann_amd import device_builder as db
    x = np.random.default_rng(n).standard_normal((n, 4)).astype(np.float32)
    got = db.kmeans(_dev(x), k, 6, 0).cpu().numpy()
    assert got.shape == (k, 4)
    np.testing.assert_array_equal(got[:n].view(np.uint32), x.view(np.uint32))
    assert np.all(got[n:] == 0)


@gpu
def test_kmeans_reseeds_with_few_distinct_rows():
    """5 distinct rows, k = 8: at least 3 centers are empty in every step and
    are re-seeded from the rows; the result stays in the rows' range."""
    from scann_amd import device_builder as db
    rng = np.random.default_rng(12)
    distinct = (5.0 * rng.standard_normal((5, 6))).astype(np.float32)
    x = distinct[rng.integers(0, 5, 200)]
    got = db.kmeans(_dev(x), 8, 6, 1).cpu().numpy()
    assert got.shape == (8, 6) and np.all(np.isfinite(got))
    assert np.all(got >= distinct.min(0)) and np.all(got <= distinct.max(0))
    # every center is one of the rows: a mean of identical rows or a re-seed
    assert all((distinct == g).all(1).any() for g in got)


def _train_codebook_ref(resid, nb, dpb, seed):
    """device_builder.train_codebook(iterations=1) on the host."""
    from scann_amd.device_builder import fixed_point_scale
    n, dim = resid.shape
    pad = np.zeros((n, nb * dpb), np.float32)
    pad[:, :dim] = resid
    blocks = pad.reshape(n, nb, dpb)
    rngs = [np.random.default_rng(seed + 7919 * b) for b in range(nb)]
    cb = np.zeros((nb, 16, dpb), np.float32)
    for b in range(nb):
        cb[b] = blocks[rngs[b].choice(n, 16, replace=False), b]
    codes = R.block_encode(resid, cb)
    scale = fixed_point_scale(float(np.abs(resid).max()), n)
    s, cnt = R.codebook_sums(resid, codes, nb, dpb, scale)
    cb = R.fixed_means(s, cnt, scale, cb.reshape(nb * 16, dpb)).reshape(nb, 16, dpb)
    cnt = cnt.reshape(nb, 16)
    for b in np.flatnonzero((cnt == 0).any(1)):
        empty = np.flatnonzero(cnt[b] == 0)
        cb[b, empty] = blocks[rngs[b].choice(n, empty.size, replace=False), b]
    return cb


@gpu
@pytest.mark.parametrize("n,dim,dpb", [(500, 21, 2), (40, 7, 3)])
def test_train_codebook_one_iteration_is_the_reference_step(n, dim, dpb):
    from scann_amd import device_builder as db
    resid = np.random.default_rng(dim).standard_normal((n, dim)).astype(np.float32)
    nb = -(-dim // dpb)
    want = _train_codebook_ref(resid, nb, dpb, seed=9)
    got = db.train_codebook(_dev(resid), nb, dpb, 1, 9).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@gpu
@pytest.mark.parametrize("n", [1, 16])
def test_train_codebook_few_rows(n):
    """n <= 16: the rows' blocks are the centers, the rest zeros."""
    from scann_amd import device_builder as db
    dim, dpb, nb = 5, 2, 3
    resid = np.random.default_rng(n).standard_normal((n, dim)).astype(np.float32)
    got = db.train_codebook(_dev(resid), nb, dpb, 4, 0).cpu().numpy()
    pad = np.zeros((n, nb * dpb), np.float32)
    pad[:, :dim] = resid
    want = np.zeros((nb, 16, dpb), np.float32)
    want[:, :n] = pad.reshape(n, nb, dpb).transpose(1, 0, 2)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _within(loss, bound, rows, leaf):
    """loss[row, leaf] is inside the bounds of the row's float64 best."""
    best = loss[rows].argmin(1)
    return loss[rows, leaf] <= loss[rows, best] + bound[rows, leaf] + bound[rows, best]


def _check_index(ix, x, oracle, soar_lambda=None, thr=None):
    """The invariants of a built TreeAHIndex, from its own arrays."""
    n = x.shape[0]
    k = ix.centers.shape[0]
    copies = 2 if soar_lambda is not None and k > 1 else 1
    off = ix.leaf_offsets.astype(np.int64)
    members = ix.leaf_members.astype(np.int64)
    m = members.size
    assert m == copies * n and off.shape == (k + 1,)
    assert off[0] == 0 and off[-1] == m and np.all(np.diff(off) >= 0)
    leaf = np.repeat(np.arange(k), np.diff(off))
    same = leaf[1:] == leaf[:-1]
    assert np.all(np.diff(members)[same] > 0)                 # ascending within a leaf
    assert np.all((members >= 0) & (members < n))
    np.testing.assert_array_equal(np.bincount(members, minlength=n), copies)
    # assignment
    loss, bound = R.kmeans_loss_bound(x, ix.centers)
    if copies == 1:
        by_id = np.empty(n, np.int64)
        by_id[members] = leaf
        assert np.all(_within(loss, bound, np.arange(n), by_id))
    else:
        order = np.lexsort((leaf, members))
        a, b = leaf[order][0::2], leaf[order][1::2]          # each id's two leaves
        assert np.all(a != b)
        rows = np.arange(n)
        ok = np.zeros(n, bool)
        for prim, sec in ((a, b), (b, a)):
            sl, sb = R.soar_loss_bound(x, ix.centers, prim.astype(np.int32), soar_lambda)
            ok |= _within(loss, bound, rows, prim) & _within(sl, sb, rows, sec)
        assert np.all(ok)
    # codes
    resid = (x[members] - ix.centers[leaf]).astype(np.float32) if ix.residual else x[members]
    if thr is None:
        want = R.block_encode(resid, ix.codebook)
    else:
        want = oracle.avq_encode(resid, x[members], ix.codebook, thr)
    np.testing.assert_array_equal(ix.member_codes, want)
    assert np.all(np.isfinite(ix.centers)) and np.all(np.isfinite(ix.codebook))


BUILD_CONFIGS = {
    # name: (n, dim, dpb, leaves, metric, kwargs)
    "dot-residual-dim21": (2000, 21, 2, 24, 0, {}),
    "l2-plain-sampled": (3000, 16, 2, 20, 1, dict(training_sample_size=1200,
                                                   ah_training_sample_size=900)),
    "soar": (1500, 12, 3, 16, 0, dict(soar_lambda=LAM)),
    "avq": (1200, 17, 2, 12, 0, dict(noise_shaping_threshold=AVQ_THR)),
}


@gpu
@pytest.mark.parametrize("name", list(BUILD_CONFIGS))
def test_build_tree_ah_index_invariants(oracle, name):
    from scann_amd import device_builder as db
    n, dim, dpb, leaves, metric, kw = BUILD_CONFIGS[name]
    x = _blobs(n, dim, 2 * leaves, seed=dim, spread=1.0, noise=0.6)
    if metric == 0:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    ix = db.build_tree_ah(x, metric, leaves, dpb, training_iterations=6,
                          ah_training_iterations=6, seed=2, **kw)
    assert ix.residual == (metric == 0) and ix.centers.shape == (leaves, dim)
    assert ix.num_blocks == -(-dim // dpb)
    _check_index(ix, x, oracle, kw.get("soar_lambda"), kw.get("noise_shaping_threshold"))


@gpu
@pytest.mark.parametrize("n,leaves", [(1, 1), (1, 4), (10, 10)])
def test_build_tree_ah_tiny(oracle, n, leaves):
    """One row; as many leaves as rows (kmeans' k >= n and train_codebook's
    n <= 16 branches inside the build)."""
    from scann_amd import device_builder as db
    x = _blobs(n, 5, 3, seed=n)
    ix = db.build_tree_ah(x, 0, leaves, 2, training_iterations=6, ah_training_iterations=6,
                          seed=1)
    assert ix.centers.shape == (min(leaves, n), 5)
    _check_index(ix, x, oracle)
    np.testing.assert_array_equal(np.sort(ix.centers, axis=0), np.sort(x, axis=0))


# ---------------------------------------------------------------------------
# unmarked: the CPU-side conditions of the tests above, and fixed_point_scale
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,k,d", R.ASSIGN_CASES, ids=_IDS)
def test_assignment_datasets_are_unambiguous(family, n, k, d):
    """The 2 % condition of both modes, and the derived bound against a
    float32 evaluation of the k-means form (an fma chain like the kernel's)."""
    x, c, _, loss, bound = _assign_case(family, n, k, d, False)
    f32 = R.kmeans_loss_f32(x, c)
    assert np.all(np.abs(f32.astype(np.float64) - loss) <= bound)
    R.check_assignment(f32.argmin(1), f32[np.arange(n), f32.argmin(1)], loss, bound)
    if k >= 2:
        _assign_case(family, n, k, d, True)


def test_assignment_edge_datasets_hold_their_conditions():
    for soar in (False, True):
        _tie_case(soar)
    _zero_residual_case()
    _kmeans_one_step_case()


def test_check_assignment_rejects_wrong_answers():
    """The checker itself: a second-best center, a loss outside the bound."""
    x, c, _, loss, bound = _assign_case("blobs", 130, 65, 65, False)
    best = loss.argmin(1)
    good = loss[np.arange(130), best].astype(np.float32)
    R.check_assignment(best, good, loss, bound)
    wrong = best.copy()
    wrong[17] = np.argsort(loss[17])[1]
    with pytest.raises(AssertionError):
        R.check_assignment(wrong, None, loss, bound)
    off = good.copy()
    off[5] += np.float32(4.0 * bound[5, best[5]] + 1e-3)
    with pytest.raises(AssertionError):
        R.check_assignment(best, off, loss, bound)


@pytest.mark.parametrize("case", [AVQ_TIE_CASE, AVQ_ROUNDS_CASE], ids=["order-tie", "rounds"])
def test_avq_special_cases_hold_their_conditions(oracle, case):
    _avq_special_case(oracle, case)


def test_fixed_point_scale_is_a_safe_power_of_two():
    from scann_amd.device_builder import fixed_point_scale
    vals = [0.0]
    for e in (-40, -1, 0, 1, 7, 30):
        p = 2.0 ** e
        vals += [p, float(np.nextafter(np.float32(p), np.float32(np.inf))),
                 float(np.nextafter(p, np.inf)), float(np.nextafter(np.float32(p), np.float32(0))),
                 p * 1.5, p * 1.9999]
    vals += [3.75, 255.0, 1e-3, 12345.678]
    for n in (1, 2, 3, 4, 1000, 4096, 4097, 2 ** 20, 2 ** 20 + 1, 10 ** 9):
        for v in vals:
            s = fixed_point_scale(v, n)
            assert R.fixed_point_scale_ok(s, v, n), (v, n, s)
            # no sum of n values of magnitude <= v can overflow int64
            assert n * (v * s + 0.5) < 2.0 ** 63


def test_codebook_lds_switch_shapes():
    """The shapes of test_codebook_mean_step_bits sit on the 64 KB switch."""
    assert codebook_lds_bytes(204, 2) == 65280 and codebook_lds_bytes(205, 2) > 65536
    assert codebook_lds_bytes(341, 1) == 65472 and codebook_lds_bytes(342, 1) > 65536
