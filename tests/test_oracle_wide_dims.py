"""The CPU oracle pinned at the widths tests/test_gpu_wide_dims.py leans on.

tests/test_oracle_kat.py derives the oracle's known answers by exact rational
arithmetic at dims 6..13 and 32 only.  The same restatements of SURVEY.md
Appendix A here, at the dims where the GPU kernels change path: the exact
reorder distance (A.8) below 8 dims, at 97..103, 104..127, 129..135 and past
136; the batched partition chains (A.10) past 128 dims for both metrics; the
lookup table (A.2/A.3) with blocks of 4 and 12 dims and a partial last block.
Every comparison is on float bits.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests.exact import F, bits, fadd, ffma, fmul, fsub, round_f32

A8_DIMS = [1, 2, 3, 5, 7, 97, 99, 101, 103, 120, 129, 130, 131, 132, 133, 134, 135, 136, 137,
           143, 200, 257]
PARTITION_DIMS = [129, 160, 161, 200]


def _term(metric, acc, a, b):
    if metric == 0:
        return ffma(-a, b, acc)
    t = fsub(a, b)
    return ffma(t, t, acc)


def _a8(q, x, metric):
    """A.8: 8 fused accumulators over whole 8-dim steps, the fold (l + 4, l),
    a 4-wide step, a 2-wide step on lanes 2 and 3, (s0 + s2) + (s1 + s3), then
    a fused scalar tail."""
    dim = len(q)
    a = [np.float32(0)] * 8
    j = 0
    while j + 8 <= dim:
        a = [_term(metric, a[l], q[j + l], x[j + l]) for l in range(8)]
        j += 8
    s = [fadd(a[l + 4], a[l]) for l in range(4)]
    if j + 4 <= dim:
        s = [_term(metric, s[l], q[j + l], x[j + l]) for l in range(4)]
        j += 4
    if j + 2 <= dim:
        s[2] = _term(metric, s[2], q[j], x[j])
        s[3] = _term(metric, s[3], q[j + 1], x[j + 1])
        j += 2
    r = fadd(fadd(s[0], s[2]), fadd(s[1], s[3]))
    if j < dim:
        r = _term(metric, r, q[j], x[j])
        j += 1
    assert j == dim
    return r


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", A8_DIMS)
def test_exact_distance_a8_at_every_tail(oracle, dim, metric):
    rng = np.random.default_rng(1000 * metric + dim)
    q = rng.standard_normal(dim).astype(np.float32)
    x = rng.standard_normal(dim).astype(np.float32)
    assert bits(oracle.exact_distance(q, x, metric)) == bits(_a8(q, x, metric))


@pytest.mark.parametrize("dim", PARTITION_DIMS)
def test_partition_dot_chain_past_128_dims(oracle, dim):
    """A.10, dot: acc <- fma(-q_d, c_d, acc) from 0, dims ascending."""
    rng = np.random.default_rng(dim)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    c = rng.standard_normal((3, dim)).astype(np.float32)
    got = oracle.partition_scores(q, c, 0)
    for i in range(2):
        for j in range(3):
            acc = np.float32(0)
            for d in range(dim):
                acc = ffma(-q[i, d], c[j, d], acc)
            assert bits(got[i, j]) == bits(acc), (dim, i, j)


def _f64(v: Fraction) -> float:
    return v.numerator / v.denominator   # int / int is correctly rounded to binary64


@pytest.mark.parametrize("dim", PARTITION_DIMS)
def test_partition_squared_l2_chain_past_128_dims(oracle, dim):
    """A.10, squared L2: ||c||^2 = -(chain acc <- fma(-c_d, c_d, acc)) in
    float; ||q||^2 accumulated in double (each square exact, each sum rounded
    to binary64) and stored as float; the accumulator starts at
    fl(||c||^2 + ||q||^2), then acc <- fma(-q_d, fl(2 c_d), acc)."""
    rng = np.random.default_rng(7 * dim)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    c = rng.standard_normal((3, dim)).astype(np.float32)
    got = oracle.partition_scores(q, c, 1)
    for i in range(2):
        s = 0.0
        for d in range(dim):
            s = _f64(Fraction(s) + F(q[i, d]) * F(q[i, d]))
        qn = round_f32(Fraction(s))
        assert bits(qn) == bits(np.float32(s))
        for j in range(3):
            cn = np.float32(0)
            for d in range(dim):
                cn = ffma(-c[j, d], c[j, d], cn)
            cn = fmul(cn, np.float32(-1.0))
            acc = fadd(cn, qn)
            for d in range(dim):
                acc = ffma(-q[i, d], fmul(c[j, d], np.float32(2.0)), acc)
            assert bits(got[i, j]) == bits(acc), (dim, i, j)


def _round_half_away(v: Fraction) -> int:
    n = int(abs(v) + Fraction(1, 2))   # floor(|v| + 1/2)
    return -n if v < 0 else n


@pytest.mark.parametrize("dim,dpb,metric", [(131, 4, 1), (768, 12, 0)])
def test_create_lut_wide_blocks(oracle, dim, dpb, metric):
    """A.2 (and A.9 for squared L2): the raw entry is the block's products
    (or squared differences) summed in coordinate order, every operation
    rounded on its own; the last block of 131 dims holds 3 of its 4.  A.3:
    m = 127 / max(sqrt(FLT_EPSILON), max|raw|), u8 = roundf(raw * m) + 128."""
    nb = -(-dim // dpb)
    last = dim - dpb * (nb - 1)
    assert (last < dpb) == (dim == 131)
    rng = np.random.default_rng(dim + dpb)
    q = rng.standard_normal(dim).astype(np.float32)
    cb = (rng.standard_normal((nb, 16, dpb)) * 0.3).astype(np.float32)
    raw, u8, m = oracle.create_lut(q, cb, metric)
    want = np.zeros((nb, 16), np.float32)
    for b in range(nb):
        nd = last if b == nb - 1 else dpb
        for k in range(16):
            s = None
            for i in range(nd):
                if metric == 0:
                    p = fmul(q[b * dpb + i], cb[b, k, i])
                else:
                    t = fsub(q[b * dpb + i], cb[b, k, i])
                    p = fmul(t, t)
                s = p if s is None else fadd(s, p)
            want[b, k] = -s if metric == 0 else s
    np.testing.assert_array_equal(raw.view(np.uint32), want.view(np.uint32))
    floor = np.sqrt(np.float32(np.finfo(np.float32).eps))
    lo = (F(np.nextafter(floor, np.float32(0))) + F(floor)) / 2
    hi = (F(floor) + F(np.nextafter(floor, np.float32(1)))) / 2
    assert lo ** 2 < F(np.finfo(np.float32).eps) < hi ** 2   # the float nearest the root
    top = max(floor, np.abs(want).max())
    assert top > floor
    mult = round_f32(Fraction(127) / F(top))
    assert bits(m) == bits(mult)
    for b in range(nb):
        for k in range(16):
            r = _round_half_away(F(fmul(want[b, k], mult)))
            assert -128 <= r <= 127
            assert int(u8[b, k]) == r + 128, (b, k)
