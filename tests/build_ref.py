"""Plain numpy / Python references of the index-build kernels
(scann_amd/csrc/smx_builder.hip, smx_sort.hip), for tests/test_gpu_build_exact.py.
Nothing here touches a GPU.

Nearest center and SOAR: float64 losses and derived float32 error bounds
---------------------------------------------------------------------------
u = 2^-24 is the float32 unit roundoff and gamma_m = m u / (1 - m u) the usual
bound on the relative error of a value that went through m roundings (Higham,
Accuracy and Stability of Numerical Algorithms, lemma 3.1).  The kernel pads
the dimension to a multiple of 32 with zeros; fma(0, 0, acc) = acc is exact,
so the padding adds no rounding.  Inputs are finite and no intermediate
underflows (the test data are O(1e-2) .. O(1e3)).

k-means form, loss_ij = ||c_j||^2 - 2 <x_i, c_j> (||x_i||^2 omitted, as
include/scann_mi355x.h documents).  The kernel forms cn = fl(sum c^2) and
acc = fl(sum x c) as fma chains of d steps (d roundings each), 2 * acc exactly,
and one subtraction: every term of the exact sum passes through at most d + 1
<= d + 2 roundings, so

    |loss_ij - LOSS_ij| <= B_ij = gamma_{d+2} (||c_j||^2 + 2 sum_t |x_it c_jt|).

SOAR form, loss_ij = ||x_i - c_j||^2 + lambda <r_i, x_i - c_j>^2 / max(||r_i||^2,
1e-30) with r_i = fl32(x_i - c_primary_i), which both sides form the same way
and which is therefore exact input data.  Upper-case names are the exact
values of the float32 inputs, lower-case the kernel's:

  * d2 = fl(fl(xx - 2 acc) + cn): xx, acc, cn are d-step fma chains, then two
    additions, so every term passes through at most d + 2 roundings:
        |d2 - D2| <= E_d2 = gamma_{d+2} (||x||^2 + 2 sum|x c| + ||c||^2);
  * proj = fl(rx - accr), rx = fl(sum r x), accr = fl(sum r c), d-step chains
    and one subtraction:
        |proj - PROJ| <= e_p = gamma_{d+1} (sum|r x| + sum|r c|),
    hence |proj^2 - PROJ^2| <= 2 |PROJ| e_p + e_p^2;
  * rr = fl(sum r^2) = RR (1 + theta_d); max(., 1e-30) is 1-Lipschitz and
    RR <= RN = max(RR, 1e-30), so rn = max(rr, 1e-30) = RN (1 + theta), |theta|
    <= gamma_d;
  * q = fl(fl(lambda fl(proj proj)) / rn) = lambda proj^2 / RN times three
    factors (1 + eps) over one factor (1 + theta_d): a relative error of at
    most gamma_{d+3} (lemma 3.1 counts the d + 3 factors), so with Q = lambda
    PROJ^2 / RN
        |q - Q| <= E_q = lambda / RN ((2 |PROJ| e_p + e_p^2) (1 + gamma_{d+3})
                                      + gamma_{d+3} PROJ^2);
  * loss = fl(d2 + q) = (d2 + q)(1 + eps):
        |loss - LOSS| <= B_ij = (E_d2 + E_q)(1 + u) + u (D2 + Q).

A row equal to its primary center bit for bit has r = 0, proj = 0 and q =
0 / 1e-30 = 0 on both sides: LOSS is the plain ||x - c_j||^2 and B = E_d2 (1 +
u) + u D2.

How the bounds are used (check_assignment): with best_i the float64 argmin,
the kernel's choice g must satisfy LOSS[i, g] <= LOSS[i, best_i] + B[i, g] +
B[i, best_i] (the kernel saw loss_g <= loss_best, each within its bound), and
the returned loss must be within B[i, g] of LOSS[i, g].  `ambiguous` marks the
rows where some other center passes that inequality; everywhere else the
kernel must return the float64 argmin exactly, and a dataset is only used if
at most 2 % of its rows are ambiguous, so the bound cannot hide a wrong
choice on more than those.

Fixed-point mean step
---------------------
S[l, j] = sum over the rows of label l of int(rint(float64(x) * scale)) (rint
and llrint both round half to even), counts from bincount, labels outside
[0, k) contribute nothing, and center = float32((float64(S) / scale) / count):
the same two IEEE divisions the kernel makes, so equality is bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24


def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


# --------------------------------------------------------------------------
# nearest center / SOAR
# --------------------------------------------------------------------------
def kmeans_loss_bound(x, c):
    """(LOSS [n, k], B [n, k]) of the k-means form, float64."""
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    cn = (c64 * c64).sum(1)[None, :]
    loss = cn - 2.0 * (x64 @ c64.T)
    bound = gamma(x.shape[1] + 2) * (cn + 2.0 * (np.abs(x64) @ np.abs(c64).T))
    return loss, bound


def soar_loss_bound(x, c, primary, lam):
    """(LOSS [n, k], B [n, k]) of the SOAR form; the primary column is +inf."""
    d = x.shape[1]
    r = (x - c[primary]).astype(np.float32).astype(np.float64)   # the kernel's float32 r
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    diff = x64[:, None, :] - c64[None, :, :]
    d2 = (diff * diff).sum(-1)
    proj = np.einsum("nd,nkd->nk", r, diff)
    rn = np.maximum((r * r).sum(1), 1e-30)[:, None]
    q = lam * proj * proj / rn
    loss = d2 + q
    xx = (x64 * x64).sum(1)[:, None]
    cn = (c64 * c64).sum(1)[None, :]
    e_d2 = gamma(d + 2) * (xx + 2.0 * (np.abs(x64) @ np.abs(c64).T) + cn)
    e_p = gamma(d + 1) * ((np.abs(r) * np.abs(x64)).sum(1)[:, None] + np.abs(r) @ np.abs(c64).T)
    g3 = gamma(d + 3)
    e_q = lam / rn * ((2.0 * np.abs(proj) * e_p + e_p * e_p) * (1.0 + g3) + g3 * proj * proj)
    bound = (e_d2 + e_q) * (1.0 + U) + U * (d2 + q)
    rows = np.arange(x.shape[0])
    loss[rows, primary] = np.inf
    bound[rows, primary] = 0.0
    return loss, bound


def ambiguous_rows(loss, bound):
    """(best [n], ambiguous [n] bool): rows where a center other than the
    float64 argmin is within the two bounds of it."""
    rows = np.arange(loss.shape[0])
    best = loss.argmin(1)
    lim = (loss[rows, best] + bound[rows, best])[:, None] + bound
    with np.errstate(invalid="ignore"):
        within = loss <= lim
    return best, within.sum(1) > 1


def check_assignment(got, got_loss, loss, bound, max_ambiguous=0.02):
    """The assertions of the module docstring, on every row."""
    n = loss.shape[0]
    rows = np.arange(n)
    best, amb = ambiguous_rows(loss, bound)
    assert amb.sum() <= max_ambiguous * n, f"{amb.sum()} of {n} rows ambiguous: dataset unusable"
    assert got.shape == (n,) and np.all((got >= 0) & (got < loss.shape[1]))
    lg, bg = loss[rows, got], bound[rows, got]
    bad = np.flatnonzero(~(lg <= loss[rows, best] + bg + bound[rows, best]))
    assert bad.size == 0, f"rows {bad[:8]}: chose {got[bad[:8]]}, float64 best {best[bad[:8]]}"
    clear = ~amb
    np.testing.assert_array_equal(got[clear], best[clear])
    if got_loss is not None:
        err = np.abs(got_loss.astype(np.float64) - lg)
        bad = np.flatnonzero(~(err <= bg))
        assert bad.size == 0, f"rows {bad[:8]}: loss error {err[bad[:8]]} > bound {bg[bad[:8]]}"


def kmeans_loss_f32(x, c):
    """The k-means form as float32 fma chains, emulated through float64: the
    product of two float32 is exact in float64, and the float64 sum rounded
    to float32 is the fma's result except where the two roundings land on a
    float32 tie (a relative 2^-53 effect, far inside the bound)."""
    n, d = x.shape
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    cn = np.zeros(c.shape[0], np.float32)
    acc = np.zeros((n, c.shape[0]), np.float32)
    for t in range(d):
        cn = (c64[:, t] * c64[:, t] + cn).astype(np.float32)
        acc = (x64[:, t, None] * c64[None, :, t] + acc).astype(np.float32)
    return (cn[None, :] - np.float32(2.0) * acc).astype(np.float32)


FAMILIES = ("blobs", "sift", "offset")


def assignment_dataset(family, n, k, d, seed, spread=1.0):
    """(x [n, d], c [k, d]) float32 of the three families: unit-normal blobs,
    SIFT-like integers 0..255, and blobs moved to +100 (where ||c||^2 - 2
    <x, c> cancels).  `spread` scales the blob centers: the SOAR form keeps
    ||x||^2, so at +100 its bound is ~ gamma_{d+2} 4 d 1e4 on every loss, and
    unit-spread centers leave the best two spilled centers inside it on far
    more than 2 % of the rows; SOAR_OFFSET_SPREAD separates them."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, n)
    if family == "sift":
        c = rng.integers(0, 256, (k, d)).astype(np.float32)
        x = np.clip(np.rint(c[lab] + 20.0 * rng.standard_normal((n, d))), 0, 255)
        return x.astype(np.float32), c
    c = spread * rng.standard_normal((k, d))
    x = c[lab] + 0.5 * rng.standard_normal((n, d))
    if family == "offset":
        c, x = c + 100.0, x + 100.0
    return x.astype(np.float32), c.astype(np.float32)


# (family, n, k, d): every n of {1, 63, 64, 65, 130}, every k of {1, 2, 3, 63,
# 64, 65, 129}, every d of {1, 2, 31, 32, 33, 65}, about 20 cases in all
ASSIGN_CASES = [
    ("blobs", 1, 1, 1), ("blobs", 63, 2, 2), ("blobs", 64, 3, 31), ("blobs", 65, 63, 32),
    ("blobs", 130, 64, 33), ("blobs", 130, 65, 65), ("blobs", 65, 129, 33),
    ("blobs", 130, 129, 1), ("blobs", 1, 129, 65), ("blobs", 64, 65, 2),
    ("sift", 130, 65, 33), ("sift", 63, 129, 65), ("sift", 65, 3, 31), ("sift", 1, 64, 32),
    ("sift", 64, 2, 31),
    ("offset", 130, 65, 65), ("offset", 65, 129, 33), ("offset", 63, 63, 32),
    ("offset", 64, 3, 31), ("offset", 1, 2, 65),
]


SOAR_OFFSET_SPREAD = 32.0


def case_seed(family, n, k, d):
    return 1000 * FAMILIES.index(family) + 7 * n + 13 * k + 31 * d


def primary_of(x, c):
    """The float64 nearest center (the SOAR tests' primary)."""
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    return ((x64[:, None, :] - c64[None]) ** 2).sum(-1).argmin(1).astype(np.int32)


# --------------------------------------------------------------------------
# fixed-point mean step
# --------------------------------------------------------------------------
def fixed_sums(x, labels, k, scale):
    """(S [k, d] int64, counts [k] int64) of the module docstring."""
    v = np.rint(x.astype(np.float64) * scale)
    assert np.all(np.abs(v) < 2.0 ** 62)
    v = v.astype(np.int64)
    ok = (labels >= 0) & (labels < k)
    s = np.zeros((k, x.shape[1]), np.int64)
    np.add.at(s, labels[ok], v[ok])
    return s, np.bincount(labels[ok], minlength=k).astype(np.int64)


def fixed_means(s, counts, scale, prev):
    """float32((float64(S) / scale) / count); empty centers keep `prev`."""
    out = np.array(prev, dtype=np.float32, copy=True)
    full = counts > 0
    mean = (s[full].astype(np.float64) / scale) / counts[full, None].astype(np.float64)
    out[full] = mean.astype(np.float32)
    return out


def codebook_sums(r, codes, nb, dpb, scale):
    """(S [nb * 16, dpb] int64, counts [nb * 16]) of smx_codebook_accumulate:
    every block's 16-center sums, the last block zero-padded."""
    n, dim = r.shape
    pad = np.zeros((n, nb * dpb), np.float32)
    pad[:, :dim] = r
    rows = pad.reshape(n * nb, dpb)
    labels = (np.arange(nb)[None, :] * 16 + codes.astype(np.int64)).reshape(-1)
    return fixed_sums(rows, labels, nb * 16, scale)


# --------------------------------------------------------------------------
# block encode, group by leaf
# --------------------------------------------------------------------------
def block_encode(r, cb):
    """smx_block_encode in float32 numpy: squared L2 over the block's
    coordinates in order, every rounding explicit, first minimum."""
    n, dim = r.shape
    nb, _, dpb = cb.shape
    pad = np.zeros((n, nb * dpb), np.float32)
    pad[:, :dim] = r
    v = (pad.reshape(n, nb, 1, dpb) - cb[None]).astype(np.float32)
    dist = np.zeros((n, nb, 16), np.float32)
    for i in range(dpb):
        dist = (dist + (v[..., i] * v[..., i]).astype(np.float32)).astype(np.float32)
    return dist.argmin(-1).astype(np.uint8)


def group_by_leaf(labels, ids_u32, k):
    """(offsets [k + 1] int64, members uint32, member leaves int32) by
    np.lexsort of (leaf, id as uint32)."""
    order = np.lexsort((ids_u32.astype(np.uint32), labels))
    off = np.zeros(k + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(labels, minlength=k))
    return off, ids_u32.astype(np.uint32)[order], labels[order].astype(np.int32)


# --------------------------------------------------------------------------
# AVQ: a Python restatement of the oracle's orc_avq_encode, only to show on
# the CPU that a test's tie really decides the codes (reverse_ties visits
# blocks of equal residual norm in the opposite order)
# --------------------------------------------------------------------------
def avq_encode_py(resid, orig, cb, threshold, reverse_ties=False, max_rounds=10):
    """(codes [n, nb] uint8, rounds [n]): rounds = passes that changed a code."""
    n, dim = resid.shape
    nb, nc, dpb = cb.shape
    out = np.zeros((n, nb), np.uint8)
    rounds = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for row in range(n):
            r = np.zeros(nb * dpb)
            x = np.zeros(nb * dpb)
            r[:dim] = resid[row]
            x[:dim] = orig[row]
            sq = np.float64(0.0)
            for j in range(nb * dpb):
                sq = sq + x[j] * x[j]
            inv = np.float64(1.0) / np.sqrt(sq)
            rn = np.zeros((nb, nc))
            par = np.zeros((nb, nc))
            for b in range(nb):
                for c in range(nc):
                    a = np.float64(0.0)
                    p = np.float64(0.0)
                    for i in range(dpb):
                        rc = r[b * dpb + i] - np.float64(cb[b, c, i])
                        a = a + rc * rc
                        p = p + rc * x[b * dpb + i] * inv
                    rn[b, c], par[b, c] = a, p
            t2 = np.float64(threshold) * np.float64(threshold)
            eta = (t2 / sq) / ((np.float64(1.0) - t2 / sq) / (np.float64(dim) - 1.0))
            code = [0] * nb
            for b in range(nb):
                best = 0
                for c in range(1, nc):
                    if rn[b, c] < rn[b, best]:
                        best = c
                code[b] = best
            P = np.float64(0.0)
            for b in range(nb):
                P = P + par[b, code[b]]
            cur = [rn[b, code[b]] for b in range(nb)]
            order = sorted(range(nb), key=lambda b: (-cur[b], -b if reverse_ties else b))
            changed = True
            rnd = 0
            while changed and rnd < max_rounds:
                changed = False
                for b in order:
                    c0 = code[b]
                    new_c, best_cost, best_p = c0, np.float64(0.0), P
                    for c in range(nc):
                        if c == c0:
                            continue
                        new_p = P - par[b, c0] + par[b, c]
                        pnd = new_p * new_p - P * P
                        if pnd > 0.0:
                            continue
                        cost = eta * pnd + ((rn[b, c] - rn[b, c0]) - pnd)
                        if cost < best_cost:
                            new_c, best_cost, best_p = c, cost, new_p
                    if new_c != c0:
                        P, code[b], changed = best_p, new_c, True
                rnd += 1
                rounds[row] += int(changed)
            out[row] = code
    return out, rounds


def fixed_point_scale_ok(scale, max_abs, n):
    """scale is a power of two with 2^60 <= n * max_abs * scale <= 2^62
    (max_abs = 0: any finite power of two)."""
    m, e = math.frexp(scale)
    if not (math.isfinite(scale) and scale > 0 and m == 0.5):
        return False
    if max_abs == 0:
        return True
    p = float(n) * float(max_abs) * scale
    return 2.0 ** 60 <= p <= 2.0 ** 62
