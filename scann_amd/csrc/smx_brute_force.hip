// smx_brute_force.hip — exact float32 brute force: the fused distance GEMM +
// top-k kernels and the smx_bf_* entry points of include/scann_mi355x.h.
//
// The batched score is that of partition_scores_kernel (smx_kernels.hip): the
// reference's brute-force searcher and its partitioner call the same
// DenseDistanceManyToManyTopK (brute_force.cc:388,
// kmeans_tree_partitioner.cc:720), so the chain acc <- fma(-q_d, x_d, acc)
// (squared L2: from fadd(xnorm, qnorm), with 2 x_d), d ascending, on
// v_mfma_f32_32x32x2_f32 is the reference's arithmetic bit for bit.
//
// The [nq][N] score matrix is never written.  The rows are taken in passes
// (the first `first_pass_rows`, each later pass kBfGrowth times the last):
//   bf_pass_kernel   64 queries x 64 rows per MFMA tile; a score whose
//                    ordered bits are <= the query's threshold tau (ties
//                    kept) goes to the query's candidate buffer as
//                    (ordered bits << 32 | row);
//   bf_fold_kernel   one block per query: candidates + running top-k sorted
//                    by (score, row), the first k kept, tau <- the k-th score.
// A query whose candidates of a pass exceed the buffer (rows sorted so that
// later ones beat earlier ones, or equal rows) is redone for that pass by its
// fold block, in pieces of at most `candidates_per_query` rows scored by the
// same FMA chain in scalar code, folding after every piece: correct for any
// row order, with nothing left to the host.  In a random order a pass that
// grows the rows seen by g keeps about g k candidates per query.
//
// The single-query search runs the same passes with the one-to-many
// accumulation of DenseDistanceOneToMany (the reorder's ExactDistance order),
// one thread per row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/scann_mi355x.h"
#include "smx_internal.h"

namespace {

using smx::kCounterStride;

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kBfTile = 64, kBfChunk = 32, kBfFullDim = 128;
constexpr int kBfBlocks = 1024;    // grid size above which a block takes several row tiles
constexpr int kBfMaxNN = 256;      // final_nn limit (kSelMax of the tree-AH select)
constexpr int kBfCapMin = 16;      // candidates_per_query limits: cap + kBfMaxNN
constexpr int kBfCapMax = 3840;    // keys are sorted in at most 32 KiB of LDS
constexpr int kBfGrowth = 4;       // rows of a pass / rows of the one before
constexpr int kBfMaxPassRows = 1 << 22;
constexpr int kBfMaxBatch = 8192;  // queries per sub-batch (bounds the workspace)
constexpr uint32_t kBfOpen = 0xFFFFFFFFu;   // tau of a query with fewer than k results

// (as smx_kernels.hip's: order-preserving float -> uint32, -0 first made +0)
__device__ __forceinline__ uint32_t BfOrderedBits(float f) {
  f = __fadd_rn(f, 0.0f);
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float BfFromOrdered(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint32_t BfNextPow2(uint32_t x) {
  return x <= 1 ? 1u : 1u << (32 - __clz(x - 1));
}

// The one-to-many accumulation (one_to_many_symmetric.h:376-503), the same
// arithmetic as ExactDistance of smx_kernels.hip: 8 fused accumulators over
// dims 0..8m-1, folded (l, l+4), a 4-wide and a 2-wide (lanes 2,3) tail, then
// (s0+s2)+(s1+s3) and a fused scalar tail.
__device__ float BfOneToMany(const float* __restrict__ q, const float* __restrict__ x, int dim,
                             int metric) {
  auto term = [metric](float acc, float a, float b) {
    if (metric == 0) return __fmaf_rn(-a, b, acc);
    const float t = __fsub_rn(a, b);
    return __fmaf_rn(t, t, acc);
  };
  float a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int j = 0;
  for (; j + 8 <= dim; j += 8) {
#pragma unroll
    for (int l = 0; l < 8; ++l) a8[l] = term(a8[l], q[j + l], x[j + l]);
  }
  float s[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) s[l] = __fadd_rn(a8[l + 4], a8[l]);
  if (j + 4 <= dim) {
#pragma unroll
    for (int l = 0; l < 4; ++l) s[l] = term(s[l], q[j + l], x[j + l]);
    j += 4;
  }
  if (j + 2 <= dim) {
    s[2] = term(s[2], q[j], x[j]);
    s[3] = term(s[3], q[j + 1], x[j + 1]);
    j += 2;
  }
  float r = __fadd_rn(__fadd_rn(s[0], s[2]), __fadd_rn(s[1], s[3]));
  if (j < dim) r = term(r, q[j], x[j]);
  return r;
}

// The batched chain of one (query, row) in scalar code: what the MFMA tile
// accumulates for that element, step for step.
__device__ float BfManyToMany(const float* __restrict__ q, const float* __restrict__ x, int dim,
                              int metric, float xnorm, float qnorm) {
  float acc = metric == 1 ? __fadd_rn(xnorm, qnorm) : 0.0f;
  const float scale = metric == 1 ? 2.0f : 1.0f;
  for (int d = 0; d < dim; ++d) acc = __fmaf_rn(-q[d], __fmul_rn(x[d], scale), acc);
  return acc;
}

// The database side's squared norms (many_to_many_impl.inc:236-257, as
// UploadIndex computes the centers'): -(acc <- fma(-x_d, x_d, acc)) in float,
// dims ascending; one thread a row.  (The query side's is a double sum,
// bf_init_kernel.)
__global__ void __launch_bounds__(256) bf_norms_kernel(const float* __restrict__ x, uint32_t n,
                                                       int dim, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = x + size_t(i) * dim;
  float acc = 0.0f;
  for (int d = 0; d < dim; ++d) acc = __fmaf_rn(-r[d], r[d], acc);
  out[i] = __fmul_rn(acc, -1.0f);
}

struct BfState {
  uint32_t* tau;      // [nq] ordered bits of the k-th score so far, or kBfOpen
  uint32_t* count;    // [nq] strided (kCounterStride): candidates of the pass
  uint32_t* have;     // [nq] results so far (<= k)
  uint64_t* top;      // [nq][k] running top-k, ascending
  uint64_t* cand;     // [nq][cap]
  uint32_t* stats;    // [0] fallback pieces [1] largest candidate count
  uint32_t cap;
};

// A call's state: open thresholds, empty lists; the squared query norms.
__global__ void __launch_bounds__(256) bf_init_kernel(const float* __restrict__ queries, int nq,
                                                      int dim, int metric, float* __restrict__ qnorm,
                                                      BfState st, int reset_stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && reset_stats) { st.stats[0] = 0u; st.stats[1] = 0u; }
  if (i >= nq) return;
  st.tau[i] = kBfOpen;
  st.count[size_t(i) * kCounterStride] = 0u;
  st.have[i] = 0u;
  if (metric == 1) {
    const float* r = queries + size_t(i) * dim;
    double s = 0.0;
    for (int d = 0; d < dim; ++d) s += double(r[d]) * double(r[d]);
    qnorm[i] = float(s);
  }
}

__device__ __forceinline__ void BfEmit(const BfState& st, int qi, uint32_t ob, uint32_t row) {
  const uint32_t p = atomicAdd(&st.count[size_t(qi) * kCounterStride], 1u);
  if (p < st.cap) st.cand[size_t(qi) * st.cap + p] = (uint64_t(ob) << 32) | row;
}

// Rows [row0, row1) against every query: a 256-thread block computes 64
// queries x 64 rows per tile (wave w: query half w & 1, row half w >> 1), the
// operands staged in LDS as partition_scores_kernel stages them (CHUNK =
// kBfFullDim, dim <= 128: the query tile once per block, the next row tile's
// loads in flight beside the MFMAs; CHUNK = kBfChunk: 32 dims a round), and
// emits the scores that pass their query's threshold.
template <int CHUNK>
__global__ void __launch_bounds__(256) bf_pass_kernel(
    const float* __restrict__ queries, int nq, int dim, const float* __restrict__ rows,
    const float* __restrict__ xnorm, const float* __restrict__ qnorm, int row0, int row1,
    int metric, BfState st, int ctiles) {
  constexpr bool kFull = CHUNK == kBfFullDim;
  __shared__ float qs[kBfTile][CHUNK + 1];
  __shared__ float cs[kBfTile][CHUNK + 1];
  __shared__ float qn[kBfTile];
  __shared__ uint32_t ts[kBfTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, k = lane >> 5;
  const int qt = blockIdx.x * kBfTile;
  const int qw = (wave & 1) * 32, cw = (wave >> 1) * 32;
  const int q0 = qt + qw;
  const int ct_first = row0 + blockIdx.y * ctiles * kBfTile;
  const int ct_end = min(row1, ct_first + ctiles * kBfTile);
  if (tid < kBfTile) {
    const int qi = qt + tid;
    // a tile row past the batch passes nothing (guarded again at the emit)
    ts[tid] = qi < nq ? st.tau[qi] : 0u;
    qn[tid] = (metric == 1 && qi < nq) ? qnorm[qi] : 0.0f;
  }
  __syncthreads();
  const float cscale = metric == 1 ? 2.0f : 1.0f;
  v16f acc;
  // C layout: col = lane & 31 (row of the database), row = (i&3) + 8*(i>>2) +
  // 4*(lane>>5) (query); this lane's 16 queries' thresholds and norms
  uint32_t tq[16];
  float qn16[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    tq[i] = ts[qw + (i & 3) + 8 * (i >> 2) + 4 * k];
    qn16[i] = qn[qw + (i & 3) + 8 * (i >> 2) + 4 * k];
  }
  auto init_acc = [&](int cbt) {
    if (metric == 1) {
      const float xn = xnorm[cbt];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = __fadd_rn(xn, qn16[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    }
  };
  auto emit = [&](int c0t) {
    const int colt = c0t + r;
    if (colt < row1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lr = (i & 3) + 8 * (i >> 2) + 4 * k;
        const uint32_t ob = BfOrderedBits(acc[i]);
        if (q0 + lr < nq && ob <= tq[i]) BfEmit(st, q0 + lr, ob, uint32_t(colt));
      }
    }
  };
  if constexpr (kFull) {
    // row tid / 4, dims tid % 4 + 4 j through one buffer resource per operand
    // that ends at the tile's last row: a read past it returns 0, and dims
    // past dim (the next row's) are masked
    constexpr int kPer = kBfFullDim / 4;
    const int row = tid >> 2, sub = tid & 3;
    const uint32_t qrows = uint32_t(min(kBfTile, nq - qt));
    const auto qrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(queries + size_t(qt) * dim), 0, int(qrows * uint32_t(dim) * 4u), 0x00020000);
    const int off = (row * dim + sub) * 4;
    float cv[kPer];
    auto load_c = [&](int ct) {
      const uint32_t crows = uint32_t(min(kBfTile, row1 - ct));
      const auto crs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(rows + size_t(ct) * dim), 0, int(crows * uint32_t(dim) * 4u), 0x00020000);
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        cv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(crs, off + 16 * j, 0, 0));
    };
    {
      float qv[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        qv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(qrs, off + 16 * j, 0, 0));
      load_c(ct_first);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int d = sub + 4 * j;
        qs[row][d] = d < dim ? -qv[j] : -0.0f;
      }
    }
    for (int cti = ct_first; cti < ct_end; cti += kBfTile) {
      if (cti != ct_first) __syncthreads();   // the previous tile's operand reads are done
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int d = sub + 4 * j;
        cs[row][d] = d < dim ? __fmul_rn(cv[j], cscale) : 0.0f;
      }
      __syncthreads();
      if (cti + kBfTile < ct_end) load_c(cti + kBfTile);
      const int c0t = cti + cw;
      init_acc(min(c0t + r, row1 - 1));
      const int steps = (dim + 15) & ~15;   // the zero padding leaves acc unchanged
      for (int s = 0; s < steps; s += 16) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          av[u] = qs[qw + r][s + 2 * u + k];
          bv[u] = cs[cw + r][s + 2 * u + k];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      }
      emit(c0t);
    }
  } else {
    for (int cti = ct_first; cti < ct_end; cti += kBfTile) {
      const int c0t = cti + cw;
      for (int d0 = 0; d0 < dim; d0 += CHUNK) {
        __syncthreads();   // the previous round's operand reads are done
        if (d0 == 0) init_acc(min(c0t + r, row1 - 1));
        constexpr int kPer = (kBfTile * CHUNK) / 256;
        float qv[kPer], cv[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
          const int e = tid + i * 256;
          const int row = e / CHUNK, col = e % CHUNK, d = min(d0 + col, dim - 1);
          qv[i] = queries[size_t(min(qt + row, nq - 1)) * dim + d];
          cv[i] = rows[size_t(min(cti + row, row1 - 1)) * dim + d];
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
          const int e = tid + i * 256;
          const int row = e / CHUNK, col = e % CHUNK, d = d0 + col;
          qs[row][col] = d < dim ? -qv[i] : -0.0f;
          cs[row][col] = d < dim ? __fmul_rn(cv[i], cscale) : 0.0f;
        }
        __syncthreads();
        const int steps = min(CHUNK, ((dim - d0) + 1) & ~1);
        for (int s = 0; s < steps; s += 2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[qw + r][s + k], cs[cw + r][s + k], acc, 0,
                                                     0, 0);
      }
      emit(c0t);
    }
  }
}

// The single query's pass: one thread a row, the one-to-many accumulation.
__global__ void __launch_bounds__(256) bf_pass_one_kernel(const float* __restrict__ query, int dim,
                                                          const float* __restrict__ rows, int row0,
                                                          int row1, int metric, BfState st) {
  const int row = row0 + int(blockIdx.x * blockDim.x + threadIdx.x);
  if (row >= row1) return;
  const uint32_t ob = BfOrderedBits(BfOneToMany(query, rows + size_t(row) * dim, dim, metric));
  if (ob <= st.tau[0]) BfEmit(st, 0, ob, uint32_t(row));
}

struct BfFoldArgs {
  BfState st;
  const float* queries;
  const float* rows;
  const float* xnorm;
  const float* qnorm;
  int dim, metric, k;
  int row0, row1;       // the pass just scored (the overflow fallback's rows)
  int one_to_many;
  int last;             // write the outputs
  uint32_t* out_idx;    // [nq][k], padded with 0
  float* out_dist;      // [nq][k], padded with NaN
  int32_t* out_count;   // [nq] or NULL
};

// Block-wide bitonic sort (ascending) of n (a power of two) keys in LDS.
__device__ void BfBitonicSort(uint64_t* keys, uint32_t n) {
  const uint32_t half = n >> 1;
  for (uint32_t k = 2; k <= n; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < half; p += blockDim.x) {
        const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));
        const uint32_t ixj = i | j;
        const uint64_t a = keys[i], b = keys[ixj];
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
          keys[i] = b;
          keys[ixj] = a;
        }
      }
      __syncthreads();
    }
  }
}

// One block per query: keys[0..have) is the running top-k, the pass's
// candidates are appended, sorted with it by (score, row) and the first k
// kept.  LDS: NextPow2(cap + k) u64 keys.
__global__ void __launch_bounds__(256) bf_fold_kernel(BfFoldArgs a) {
  extern __shared__ uint64_t keys[];
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x, qi = blockIdx.x;
  const BfState& st = a.st;
  const uint32_t cap = st.cap, k = uint32_t(a.k);
  const uint32_t n = st.count[size_t(qi) * kCounterStride];
  uint32_t have = st.have[qi];
  uint64_t* top = st.top + size_t(qi) * k;
  for (uint32_t i = tid; i < have; i += 256) keys[i] = top[i];
  // sorts keys[0..have + m) and keeps the first k; returns the new threshold
  auto fold = [&](uint32_t m) {
    const uint32_t tot = have + m, np2 = BfNextPow2(tot);
    for (uint32_t i = tot + tid; i < np2; i += 256) keys[i] = ~0ull;
    __syncthreads();
    BfBitonicSort(keys, np2);
    have = min(k, tot);
    return have == k ? uint32_t(keys[k - 1] >> 32) : kBfOpen;
  };
  uint32_t tau;
  if (n <= cap) {
    const uint64_t* cand = st.cand + size_t(qi) * cap;
    for (uint32_t i = tid; i < n; i += 256) keys[have + i] = cand[i];
    tau = fold(n);
  } else {
    // more candidates than the buffer holds: this pass again for this query,
    // cap rows at a time (at most cap candidates), tau tightened after each
    tau = st.tau[qi];
    const float* q = a.queries + size_t(qi) * a.dim;
    const float qnorm = (a.metric == 1 && !a.one_to_many) ? a.qnorm[qi] : 0.0f;
    uint32_t pieces = 0;
    for (int p0 = a.row0; p0 < a.row1; p0 += int(cap), ++pieces) {
      if (tid == 0) s_n = 0u;
      __syncthreads();
      const int p1 = min(a.row1, p0 + int(cap));
      for (int row = p0 + tid; row < p1; row += 256) {
        const float* x = a.rows + size_t(row) * a.dim;
        const float sc = a.one_to_many
                             ? BfOneToMany(q, x, a.dim, a.metric)
                             : BfManyToMany(q, x, a.dim, a.metric,
                                            a.metric == 1 ? a.xnorm[row] : 0.0f, qnorm);
        const uint32_t ob = BfOrderedBits(sc);
        if (ob <= tau) keys[have + atomicAdd(&s_n, 1u)] = (uint64_t(ob) << 32) | uint32_t(row);
      }
      __syncthreads();
      const uint32_t m = s_n;
      tau = fold(m);
      __syncthreads();   // every thread has read s_n and keys[k - 1]
    }
    if (tid == 0) atomicAdd(&st.stats[0], pieces);
  }
  for (uint32_t i = tid; i < have; i += 256) top[i] = keys[i];
  if (tid == 0) {
    st.tau[qi] = tau;
    st.have[qi] = have;
    st.count[size_t(qi) * kCounterStride] = 0u;
    atomicMax(&st.stats[1], n);
    if (a.last && a.out_count) a.out_count[qi] = int32_t(have);
  }
  if (a.last) {
    for (uint32_t i = tid; i < k; i += 256) {
      const bool has = i < have;
      a.out_idx[size_t(qi) * k + i] = has ? uint32_t(keys[i] & 0xFFFFFFFFu) : 0u;
      a.out_dist[size_t(qi) * k + i] =
          has ? BfFromOrdered(uint32_t(keys[i] >> 32)) : __int_as_float(0x7fc00000);
    }
  }
}

int Fail(int code, const std::string& msg) { return smx::SetLastError(code, msg); }

#define BF_HIP(expr)                                                               \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return Fail(_e == hipErrorOutOfMemory ? SMX_OUT_OF_MEMORY : SMX_DEVICE_ERROR, \
                  std::string("HIP error in ") + #expr + ": " + hipGetErrorString(_e)); \
  } while (0)

template <typename T>
void BfFree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

struct smx_bf {
  int device = 0, metric = 0, dim = 0;
  uint32_t n = 0;
  // the only buffers proportional to N: the rows and their squared norms
  float* rows = nullptr;     // [n][dim]
  float* xnorm = nullptr;    // [n], squared L2 only
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;   // of the last search (smx_bf_get_stats waits for it)
  mutable std::mutex mu;
  int first_pass_rows = 0, candidates = 0;   // tuning, 0 = default
  int passes = 0;                            // of the last call
  // Per-call workspace, for nq_cap <= kBfMaxBatch queries of a sub-batch and
  // cap <= kBfCapMax candidates each -- bytes:
  //   nq_cap * (8 cap [cand] + 8 kBfMaxNN [top] + 4 kCounterStride [count]
  //             + 12 [tau, have, qnorm])
  //   + for the host-buffer calls nq_cap * (4 dim [queries] + 8 kBfMaxNN + 4 [outputs]),
  // at most 8192 * (30720 + 2048 + 128 + 12) = 270 MB whatever N is.
  int nq_cap = 0;
  size_t cand_elems = 0;
  BfState st{};
  float* qnorm = nullptr;
  float* h_queries = nullptr;   // host-buffer calls: [nq_cap][dim]
  uint32_t* h_idx = nullptr;    // [nq_cap][kBfMaxNN]
  float* h_dist = nullptr;
  int32_t* h_count = nullptr;
};

namespace {

void FreeWorkspace(smx_bf* h) {
  BfFree(h->st.tau);
  BfFree(h->st.count);
  BfFree(h->st.have);
  BfFree(h->st.top);
  BfFree(h->st.cand);
  BfFree(h->qnorm);
  BfFree(h->h_queries);
  BfFree(h->h_idx);
  BfFree(h->h_dist);
  BfFree(h->h_count);
  h->nq_cap = 0;
  h->cand_elems = 0;
}

int CapFor(const smx_bf* h, int k) {
  if (h->candidates) return h->candidates;
  // a pass that grows the rows seen kBfGrowth-fold keeps ~kBfGrowth k of a
  // random order's rows per query: four times that
  return std::min(kBfCapMax, std::max(1024, 4 * kBfGrowth * k));
}

int EnsureWorkspace(smx_bf* h, int nq, int cap, bool host) {
  if (nq > h->nq_cap) {
    // (the stats words survive: they are allocated with the handle)
    uint32_t* stats = h->st.stats;
    BF_HIP(hipDeviceSynchronize());
    FreeWorkspace(h);
    h->st.stats = stats;
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->st.tau), sizeof(uint32_t) * nq));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->st.count), sizeof(uint32_t) * kCounterStride * nq));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->st.have), sizeof(uint32_t) * nq));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->st.top), sizeof(uint64_t) * kBfMaxNN * nq));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->qnorm), sizeof(float) * nq));
    h->nq_cap = nq;
  }
  const size_t need = size_t(h->nq_cap) * cap;
  if (need > h->cand_elems) {
    BF_HIP(hipDeviceSynchronize());
    BfFree(h->st.cand);
    h->cand_elems = 0;
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->st.cand), sizeof(uint64_t) * need));
    h->cand_elems = need;
  }
  if (host && !h->h_queries) {
    const size_t q = size_t(h->nq_cap);
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->h_queries), sizeof(float) * q * h->dim));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->h_idx), sizeof(uint32_t) * q * kBfMaxNN));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->h_dist), sizeof(float) * q * kBfMaxNN));
    BF_HIP(hipMalloc(reinterpret_cast<void**>(&h->h_count), sizeof(int32_t) * q));
  }
  return SMX_OK;
}

// One sub-batch (nq <= nq_cap) on stream s: init, then a pass and a fold per
// slab of rows.  `first` resets the call's stats.
int RunBf(smx_bf* h, const float* dq, int nq, int k, bool one, bool first, uint32_t* d_idx,
          float* d_dist, int32_t* d_count, hipStream_t s) {
  // one workspace: a call on another stream than the last one's waits for it
  if (h->last_stream && h->last_stream != s) BF_HIP(hipStreamSynchronize(h->last_stream));
  const int cap = CapFor(h, k);
  BfState st = h->st;
  st.cap = uint32_t(cap);
  hipLaunchKernelGGL(bf_init_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, dq, nq, h->dim,
                     h->metric, h->qnorm, st, first ? 1 : 0);
  const int n = int(h->n);
  // the first pass passes every row (open thresholds): at most cap of them
  int size = h->first_pass_rows ? h->first_pass_rows : cap;
  const size_t lds = sizeof(uint64_t) * size_t(1u << (32 - __builtin_clz(unsigned(cap + k - 1))));
  const int qtiles = (nq + kBfTile - 1) / kBfTile;
  int passes = 0;
  for (int row0 = 0; row0 < n; ++passes) {
    const int row1 = int(std::min<int64_t>(n, int64_t(row0) + size));
    if (one) {
      hipLaunchKernelGGL(bf_pass_one_kernel, dim3((row1 - row0 + 255) / 256), dim3(256), 0, s, dq,
                         h->dim, h->rows, row0, row1, h->metric, st);
    } else {
      const int ctl = (row1 - row0 + kBfTile - 1) / kBfTile;
      const int per = std::max(1, (qtiles * ctl + kBfBlocks - 1) / kBfBlocks);
      const dim3 grid(qtiles, (ctl + per - 1) / per);
      if (h->dim <= kBfFullDim)
        hipLaunchKernelGGL(bf_pass_kernel<kBfFullDim>, grid, dim3(256), 0, s, dq, nq, h->dim,
                           h->rows, h->xnorm, h->qnorm, row0, row1, h->metric, st, per);
      else
        hipLaunchKernelGGL(bf_pass_kernel<kBfChunk>, grid, dim3(256), 0, s, dq, nq, h->dim, h->rows,
                           h->xnorm, h->qnorm, row0, row1, h->metric, st, per);
    }
    BfFoldArgs a{};
    a.st = st;
    a.queries = dq;
    a.rows = h->rows;
    a.xnorm = h->xnorm;
    a.qnorm = h->qnorm;
    a.dim = h->dim;
    a.metric = h->metric;
    a.k = k;
    a.row0 = row0;
    a.row1 = row1;
    a.one_to_many = one ? 1 : 0;
    a.last = row1 == n ? 1 : 0;
    a.out_idx = d_idx;
    a.out_dist = d_dist;
    a.out_count = d_count;
    hipLaunchKernelGGL(bf_fold_kernel, dim3(nq), dim3(256), lds, s, a);
    row0 = row1;
    size = int(std::min<int64_t>(kBfMaxPassRows, int64_t(size) * kBfGrowth));
  }
  BF_HIP(hipGetLastError());
  if (first) h->passes = passes;
  h->last_stream = s;
  return SMX_OK;
}

int CheckArgs(const smx_bf* h, int nq, int dim, int final_nn) {
  if (!h) return Fail(SMX_INVALID_ARGUMENT, "null brute-force handle");
  if (nq < 0) return Fail(SMX_INVALID_ARGUMENT, "negative batch size");
  if (dim != h->dim) return Fail(SMX_INVALID_ARGUMENT, "Query doesn't match dataset dimsensionality");
  if (final_nn <= 0) return Fail(SMX_INVALID_ARGUMENT, "final_num_neighbors must be > 0");
  if (final_nn > kBfMaxNN)
    return Fail(SMX_INVALID_ARGUMENT, "final_num_neighbors above 256 is not supported by the "
                                      "brute-force searcher");
  return SMX_OK;
}

int SearchDevice(smx_bf* h, const float* dq, int nq, int k, bool one, uint32_t* d_idx, float* d_dist,
                 int32_t* d_count, hipStream_t s) {
  const int cap = CapFor(h, k);
  int rc = EnsureWorkspace(h, std::min(nq, kBfMaxBatch), cap, false);
  if (rc) return rc;
  for (int b = 0; b < nq; b += kBfMaxBatch) {
    const int m = std::min(kBfMaxBatch, nq - b);
    rc = RunBf(h, dq + size_t(b) * h->dim, m, k, one, b == 0, d_idx + size_t(b) * k,
               d_dist + size_t(b) * k, d_count ? d_count + b : nullptr, s);
    if (rc) return rc;
  }
  return SMX_OK;
}

int SearchHost(smx_bf* h, const float* queries, int nq, int dim, int k, bool one, uint32_t* out_idx,
               float* out_dist, int32_t* out_count) {
  int rc = CheckArgs(h, nq, dim, k);
  if (rc) return rc;
  if (nq == 0) return SMX_OK;
  if (!queries || !out_idx || !out_dist)
    return Fail(SMX_INVALID_ARGUMENT, "null query or output buffer");
  for (size_t i = 0; i < size_t(nq) * dim; ++i)
    if (!std::isfinite(queries[i])) return Fail(SMX_INVALID_ARGUMENT, "queries must be finite");
  std::lock_guard<std::mutex> lock(h->mu);
  BF_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if ((rc = EnsureWorkspace(h, std::min(nq, kBfMaxBatch), CapFor(h, k), true))) return rc;
  for (int b = 0; b < nq; b += kBfMaxBatch) {
    const int m = std::min(kBfMaxBatch, nq - b);
    BF_HIP(hipMemcpyAsync(h->h_queries, queries + size_t(b) * dim, sizeof(float) * size_t(m) * dim,
                          hipMemcpyHostToDevice, s));
    if ((rc = RunBf(h, h->h_queries, m, k, one, b == 0, h->h_idx, h->h_dist, h->h_count, s)))
      return rc;
    BF_HIP(hipMemcpyAsync(out_idx + size_t(b) * k, h->h_idx, sizeof(uint32_t) * size_t(m) * k,
                          hipMemcpyDeviceToHost, s));
    BF_HIP(hipMemcpyAsync(out_dist + size_t(b) * k, h->h_dist, sizeof(float) * size_t(m) * k,
                          hipMemcpyDeviceToHost, s));
    if (out_count)
      BF_HIP(hipMemcpyAsync(out_count + b, h->h_count, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
    BF_HIP(hipStreamSynchronize(s));
  }
  return SMX_OK;
}

}  // namespace

extern "C" {

int smx_bf_create(const smx_bf_desc* d, int32_t device, smx_bf** out) {
  if (!out) return Fail(SMX_INVALID_ARGUMENT, "null output handle");
  *out = nullptr;
  if (!d) return Fail(SMX_INVALID_ARGUMENT, "null description");
  if (d->metric != SMX_METRIC_DOT && d->metric != SMX_METRIC_SQUARED_L2)
    return Fail(SMX_INVALID_ARGUMENT, "unknown metric");
  if (d->dim < 1 || d->dim > (1 << 20)) return Fail(SMX_INVALID_ARGUMENT, "dim must be in [1, 2^20]");
  if (d->num_datapoints == 0 || !d->dataset) return Fail(SMX_INVALID_ARGUMENT, "empty dataset");
  // row indices are ints in the kernels; a 64-row tile's bytes fit a buffer resource
  if (d->num_datapoints > 0x7FFFFF00u) return Fail(SMX_INVALID_ARGUMENT, "more than 2^31 - 256 rows");
  int ndev = 0;
  BF_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return Fail(SMX_INVALID_ARGUMENT, "no such HIP device");
  BF_HIP(hipSetDevice(device));
  auto* h = new smx_bf;
  h->device = device;
  h->metric = d->metric;
  h->dim = d->dim;
  h->n = d->num_datapoints;
  const size_t elems = size_t(h->n) * h->dim;
  auto fail = [&](int code, const char* msg) {
    smx_bf_destroy(h);
    return Fail(code, msg);
  };
  if (hipMalloc(reinterpret_cast<void**>(&h->rows), sizeof(float) * elems) != hipSuccess)
    return fail(SMX_OUT_OF_MEMORY, "hipMalloc of the dataset failed");
  if (hipMalloc(reinterpret_cast<void**>(&h->st.stats), sizeof(uint32_t) * 4) != hipSuccess)
    return fail(SMX_OUT_OF_MEMORY, "hipMalloc failed");
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(SMX_DEVICE_ERROR, "hipStreamCreate failed");
  if (hipMemcpyAsync(h->rows, d->dataset, sizeof(float) * elems, hipMemcpyHostToDevice, h->stream) !=
          hipSuccess ||
      hipMemsetAsync(h->st.stats, 0, sizeof(uint32_t) * 4, h->stream) != hipSuccess)
    return fail(SMX_DEVICE_ERROR, "dataset upload failed");
  if (h->metric == SMX_METRIC_SQUARED_L2) {
    if (hipMalloc(reinterpret_cast<void**>(&h->xnorm), sizeof(float) * h->n) != hipSuccess)
      return fail(SMX_OUT_OF_MEMORY, "hipMalloc of the row norms failed");
    hipLaunchKernelGGL(bf_norms_kernel, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->rows,
                       h->n, h->dim, h->xnorm);
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return fail(SMX_DEVICE_ERROR, "dataset upload failed");
  *out = h;
  return SMX_OK;
}

int smx_bf_destroy(smx_bf* h) {
  if (!h) return SMX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  FreeWorkspace(h);
  BfFree(h->st.stats);
  BfFree(h->rows);
  BfFree(h->xnorm);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return SMX_OK;
}

int smx_bf_search_batched(smx_bf* h, const float* queries, int32_t nq, int32_t dim, int32_t final_nn,
                          uint32_t* out_idx, float* out_dist, int32_t* out_count) {
  return SearchHost(h, queries, nq, dim, final_nn, false, out_idx, out_dist, out_count);
}

int smx_bf_search_batched_device(smx_bf* h, const float* d_queries, int32_t nq, int32_t dim,
                                 int32_t final_nn, uint32_t* d_out_idx, float* d_out_dist,
                                 int32_t* d_out_count, void* stream) {
  int rc = CheckArgs(h, nq, dim, final_nn);
  if (rc) return rc;
  if (nq == 0) return SMX_OK;
  if (!d_queries || !d_out_idx || !d_out_dist)
    return Fail(SMX_INVALID_ARGUMENT, "null query or output buffer");
  std::lock_guard<std::mutex> lock(h->mu);
  BF_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  return SearchDevice(h, d_queries, nq, final_nn, false, d_out_idx, d_out_dist, d_out_count, s);
}

int smx_bf_search(smx_bf* h, const float* query, int32_t dim, int32_t final_nn, uint32_t* out_idx,
                  float* out_dist, int32_t* out_count) {
  return SearchHost(h, query, 1, dim, final_nn, true, out_idx, out_dist, out_count);
}

int smx_bf_set_tuning(smx_bf* h, int32_t first_pass_rows, int32_t candidates_per_query) {
  if (!h) return Fail(SMX_INVALID_ARGUMENT, "null brute-force handle");
  if (first_pass_rows < 0 || first_pass_rows > kBfMaxPassRows)
    return Fail(SMX_INVALID_ARGUMENT, "first_pass_rows must be 0 (default) or in [1, 2^22]");
  if (candidates_per_query != 0 &&
      (candidates_per_query < kBfCapMin || candidates_per_query > kBfCapMax))
    return Fail(SMX_INVALID_ARGUMENT, "candidates_per_query must be 0 (default) or in [16, 3840]");
  std::lock_guard<std::mutex> lock(h->mu);
  h->first_pass_rows = first_pass_rows;
  h->candidates = candidates_per_query;
  return SMX_OK;
}

int smx_bf_get_stats(const smx_bf* h, smx_bf_stats* out) {
  if (!h || !out) return Fail(SMX_INVALID_ARGUMENT, "null handle or output");
  std::lock_guard<std::mutex> lock(h->mu);
  BF_HIP(hipSetDevice(h->device));
  if (h->last_stream) BF_HIP(hipStreamSynchronize(h->last_stream));
  uint32_t w[2] = {0, 0};
  BF_HIP(hipMemcpy(w, h->st.stats, sizeof(w), hipMemcpyDeviceToHost));
  out->passes = h->passes;
  out->fallback_pieces = int32_t(w[0]);
  out->max_candidates = int32_t(w[1]);
  out->reserved = 0;
  return SMX_OK;
}

}  // extern "C"
