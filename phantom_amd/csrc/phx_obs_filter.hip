// phx_obs_filter.hip -- phx_filter_update / phx_filter_apply (include/phantom_amd_filter.h): a running mean and M2 of every
// observation feature per class, folded a fragment at a time in the header's fixed order, and the pass that normalises a plane with
// them.  No atomics and no grid-wide barrier: the order of every f64 add is the header's.
//
// phx_filter_update is five launches on one stream:
//   phx_filter_sum_kernel     a lane owns ONE column and a wave 64 consecutive ones (phx_episodes.hip's mapping): the D floats of a
//                             column element are contiguous, so a wave's row access is one piece of 64 * D floats.  The rows are
//                             consumed FC rows at a time: a chunk's loads (rows past T clamped to T - 1, never branched around) are
//                             issued before its adds.  D is a template parameter: the D sums stay in registers.  Writes s_n[d] to
//                             the workspace as [D][N] (the fold reads it with unit stride) and the column's kept count.
//   phx_filter_mean_kernel    one 256-lane workgroup per (class, feature): lane i folds n = i, i + 256, .. ascending from +0.0
//                             (columns of other classes: skipped, which equals adding +0.0; FL_K columns are loaded ahead of their
//                             adds), then the halving tree over LDS; the kept count K_c is the exact integer sum.  Writes mb = sum / K
//                             and K to the workspace's table.
//   phx_filter_center_kernel  the sum kernel's walk again with q_n += (x - mb) * (x - mb), mb of the column's class from the table.
//   phx_filter_m2_kernel      the same fold over q_n: M2b to the table.
//   phx_filter_merge_kernel   ONE workgroup of 256 = 16 classes x 16 features: every lane reads its class's count, a barrier, then Chan's
//                             merge of its (class, feature); lane d == 0 of a class writes count and updates.  No kernel reads a state
//                             field another one of the call writes, and inside the merge every read of count precedes the barrier.
// phx_filter_apply is one launch, phx_filter_apply_kernel: the plane as a flat run of 16-byte pieces (obs and out are 16-byte aligned, so
// every piece is, whatever N and D; a last piece of fewer than four floats goes element by element).  A workgroup owns FA_U * 256
// consecutive pieces: it builds the (mean_f, den_f, clip) table of every (class, feature) in LDS from the state at entry, splits its
// first float's index into (row, position in the row) once, and a thread then issues ALL its loads -- FA_U pieces with the keep bytes
// and classes of their elements -- before its first store (loads and stores share vmcnt on gfx950): no load follows a
// store.  In place (out == obs) a thread reads exactly the pieces it writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_filter.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int FL_LANES = 64;         // columns per workgroup of the two column walks: one wave
constexpr int FL_RED = 256;          // the folds' workgroup: the header's 256 lane values
constexpr int FL_K = 8;              // columns a lane of a fold loads ahead of its adds (a chain of dependent loads otherwise)
constexpr int FL_MD = PHX_FILTER_MAX_DIM;
constexpr int FL_MC = PHX_FILTER_MAX_CLASSES;
constexpr int FA_THREADS = 256;      // the apply's workgroup
constexpr int FA_U = 4;              // 16-byte pieces per thread of the apply
constexpr int64_t FA_CHUNK = (int64_t)FA_THREADS * FA_U * 4;      // floats per workgroup of the apply

typedef float fl_f32x4 __attribute__((ext_vector_type(4)));

// rows per chunk of a column walk: FC * D element loads and FC keep loads in flight per lane
template <int D>
constexpr int fl_rows() { return D <= 4 ? 8 : (D <= 8 ? 4 : 2); }

// the workspace (doubles): [D][N] per-column partials, [N] kept counts (as int64), then the table: mb[16][16], M2b[16][16], K[16] (int64)
struct FlWork {
  double* part;
  int64_t* cnt;
  double* mb;
  double* m2b;
  int64_t* K;
};

static __host__ __device__ __forceinline__ FlWork fl_work(double* ws, const int64_t N, const int D) {
  FlWork w;
  w.part = ws;
  w.cnt = reinterpret_cast<int64_t*>(ws + (int64_t)D * N);
  w.mb = ws + (int64_t)(D + 1) * N;
  w.m2b = w.mb + FL_MC * FL_MD;
  w.K = reinterpret_cast<int64_t*>(w.m2b + FL_MC * FL_MD);
  return w;
}

// the walk of one column: CENTRED = false sums x, CENTRED = true sums (x - mb) * (x - mb) with the class's mb
template <int D, bool HAS_KEEP, bool CENTRED>
__device__ __forceinline__ void fl_walk(const phx_filter_update_io& a, const int64_t n, double (&acc)[D], int64_t& kept) {
  constexpr int FC = fl_rows<D>();
  double mb[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    acc[d] = 0.0;
    mb[d] = 0.0;
  }
  kept = 0;
  if (CENTRED) {
    const int cls = a.col_class ? a.col_class[n] : 0;
    if (cls < 0 || cls >= a.n_classes) return;           // (a column of no class enters no fold)
    const FlWork w = fl_work(a.workspace, a.N, D);
#pragma unroll
    for (int d = 0; d < D; ++d) mb[d] = w.mb[cls * FL_MD + d];
  }
  for (int t0 = 0; t0 < a.T; t0 += FC) {
    float x[FC][D];
    uint32_t k[FC];
#pragma unroll
    for (int r = 0; r < FC; ++r) {                       // the chunk's loads, rows past the last clamped to it
      const int t = t0 + r < a.T ? t0 + r : a.T - 1;
      const int64_t o = (int64_t)t * a.N + n;
      if (HAS_KEEP) k[r] = a.keep[o];
#pragma unroll
      for (int d = 0; d < D; ++d) x[r][d] = a.obs[o * D + d];
    }
#pragma unroll
    for (int r = 0; r < FC; ++r) {
      const bool on = t0 + r < a.T && (!HAS_KEEP || k[r] != 0);
      kept += on ? 1 : 0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double v = (double)x[r][d];
        const double c = v - mb[d];
        const double term = CENTRED ? c * c : v;
        acc[d] = on ? acc[d] + term : acc[d];
      }
    }
  }
}

template <int D, bool HAS_KEEP>
__global__ __launch_bounds__(FL_LANES) void phx_filter_sum_kernel(const phx_filter_update_io a) {
  const int64_t n = (int64_t)blockIdx.x * FL_LANES + threadIdx.x;
  if (n >= a.N) return;
  double acc[D];
  int64_t kept;
  fl_walk<D, HAS_KEEP, false>(a, n, acc, kept);
  const FlWork w = fl_work(a.workspace, a.N, D);
#pragma unroll
  for (int d = 0; d < D; ++d) w.part[(int64_t)d * a.N + n] = acc[d];
  w.cnt[n] = kept;
}

template <int D, bool HAS_KEEP>
__global__ __launch_bounds__(FL_LANES) void phx_filter_center_kernel(const phx_filter_update_io a) {
  const int64_t n = (int64_t)blockIdx.x * FL_LANES + threadIdx.x;
  if (n >= a.N) return;
  double acc[D];
  int64_t kept;
  fl_walk<D, HAS_KEEP, true>(a, n, acc, kept);
  const FlWork w = fl_work(a.workspace, a.N, D);
#pragma unroll
  for (int d = 0; d < D; ++d) w.part[(int64_t)d * a.N + n] = acc[d];
}

// the header's fixed order over the columns of class `cls`, feature d: the f64 sum of part[d][n] and the exact kept count
__device__ __forceinline__ void fl_fold(const phx_filter_update_io& a, const FlWork& w, const int cls, const int d, double& sum, int64_t& K) {
  __shared__ double ls[FL_RED];
  __shared__ int64_t lk[FL_RED];
  const int i = (int)threadIdx.x;
  const double* part = w.part + (int64_t)d * a.N;
  double s = 0.0;
  int64_t k = 0;
  for (int64_t j0 = i; j0 < a.N; j0 += (int64_t)FL_K * FL_RED) {       // (FL_K columns loaded ahead of their adds; the adds in the header's order)
    double v[FL_K];
    int64_t kc[FL_K];
    int c[FL_K];
#pragma unroll
    for (int u = 0; u < FL_K; ++u) {
      const int64_t j = j0 + (int64_t)u * FL_RED;
      const int64_t jc = j < a.N ? j : a.N - 1;
      c[u] = a.col_class ? a.col_class[jc] : 0;
      v[u] = part[jc];
      kc[u] = w.cnt[jc];
    }
#pragma unroll
    for (int u = 0; u < FL_K; ++u) {
      const bool in = j0 + (int64_t)u * FL_RED < a.N && c[u] == cls;
      s = in ? s + v[u] : s;
      k += in ? kc[u] : 0;
    }
  }
  ls[i] = s;
  lk[i] = k;
  __syncthreads();
  for (int h = FL_RED / 2; h >= 1; h >>= 1) {
    if (i < h) {
      s = s + ls[i + h];
      k += lk[i + h];
      ls[i] = s;
      lk[i] = k;
    }
    __syncthreads();
  }
  sum = s;
  K = k;
}

__global__ __launch_bounds__(FL_RED) void phx_filter_mean_kernel(const phx_filter_update_io a) {
  const int cls = (int)blockIdx.x / a.D, d = (int)blockIdx.x % a.D;
  const FlWork w = fl_work(a.workspace, a.N, a.D);
  double sum;
  int64_t K;
  fl_fold(a, w, cls, d, sum, K);
  if (threadIdx.x == 0) {
    w.mb[cls * FL_MD + d] = K > 0 ? sum / (double)K : 0.0;
    if (d == 0) w.K[cls] = K;
  }
}

__global__ __launch_bounds__(FL_RED) void phx_filter_m2_kernel(const phx_filter_update_io a) {
  const int cls = (int)blockIdx.x / a.D, d = (int)blockIdx.x % a.D;
  const FlWork w = fl_work(a.workspace, a.N, a.D);
  double sum;
  int64_t K;
  fl_fold(a, w, cls, d, sum, K);
  if (threadIdx.x == 0) w.m2b[cls * FL_MD + d] = sum;
}

__global__ __launch_bounds__(FL_MC* FL_MD) void phx_filter_merge_kernel(const phx_filter_update_io a) {
  const int cls = (int)threadIdx.x / FL_MD, d = (int)threadIdx.x % FL_MD;
  const bool mine = cls < a.n_classes && d < a.D;
  const FlWork w = fl_work(a.workspace, a.N, a.D);
  int64_t na = 0, K = 0;
  if (mine) {
    na = a.state[cls].count;
    K = w.K[cls];
  }
  __syncthreads();                                       // every read of count is behind us: lane d == 0 may write it
  if (!mine || K == 0) return;                           // (an empty class keeps its bytes, `updates` included)
  const int64_t n = na + K;
  const double mb = w.mb[cls * FL_MD + d], m2b = w.m2b[cls * FL_MD + d];
  const double mean = a.state[cls].mean[d], m2 = a.state[cls].m2[d];
  const double delta = mb - mean;
  a.state[cls].mean[d] = mean + delta * ((double)K / (double)n);
  a.state[cls].m2[d] = (m2 + m2b) + (delta * delta) * (((double)na * (double)K) / (double)n);
  if (d == 0) {
    a.state[cls].count = n;
    a.state[cls].updates += 1;
  }
}

struct FaEntry {
  float mean, den, clip;                                 // clip == 0: none
};

// one float of the plane: its element's keep byte and class were loaded as k and c
__device__ __forceinline__ float fa_one(const FaEntry* tab, const float x, const uint32_t k, const int c, const int d, const int n_classes) {
  if (k == 0 || c < 0 || c >= n_classes) return 0.0f;
  const FaEntry e = tab[c * FL_MD + d];
  float y = (x - e.mean) / e.den;
  if (e.clip > 0.0f) y = fminf(fmaxf(y, -e.clip), e.clip);
  return y;
}

template <int D>
__global__ __launch_bounds__(FA_THREADS) void phx_filter_apply_kernel(const phx_filter_apply_io a, const int64_t E) {
  __shared__ FaEntry tab[FL_MC * FL_MD];
  {
    const int cls = (int)threadIdx.x / FL_MD, d = (int)threadIdx.x % FL_MD;
    FaEntry e;
    e.mean = 0.0f;
    e.den = 1.0f;
    e.clip = 0.0f;
    if (cls < a.n_classes && d < D) {
      const int64_t count = a.state[cls].count;
      const double mean = a.state[cls].mean[d], m2 = a.state[cls].m2[d];
      if (count > 0) {
        const double var = count == 1 ? mean * mean : m2 / (double)(count - 1);
        e.mean = (float)mean;
        e.den = (float)__builtin_sqrt(var) + 1e-8f;
        e.clip = a.clip;
      }
    }
    tab[threadIdx.x] = e;
  }
  __syncthreads();
  const uint32_t L = (uint32_t)(a.N * D);                // floats per row (the launcher keeps L + FA_CHUNK below 2^32)
  const int64_t e_base = (int64_t)blockIdx.x * FA_CHUNK;
  const int64_t t_base = e_base / L;
  const uint32_t f_base = (uint32_t)(e_base - t_base * L);
  fl_f32x4 x[FA_U];
  uint32_t k[FA_U][4];
  int c[FA_U][4], dd[FA_U][4];
#pragma unroll
  for (int u = 0; u < FA_U; ++u) {                       // every load of the thread, before its first store
    const uint32_t o = ((uint32_t)u * FA_THREADS + threadIdx.x) * 4u;
    const int64_t e0 = e_base + o;
    const uint32_t g = f_base + o;
    const uint32_t dt = g / L;
    uint32_t f = g - dt * L;
    int64_t t = t_base + dt;
    uint32_t n = f / (uint32_t)D;
    int d = (int)(f - n * (uint32_t)D);
    const bool whole = e0 + 4 <= E;
    if (whole) {
      x[u] = *reinterpret_cast<const fl_f32x4*>(a.obs + e0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[u][j] = e0 + j < E ? a.obs[e0 + j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e0 + j < E;
      k[u][j] = in ? (a.keep ? (uint32_t)a.keep[t * a.N + n] : 1u) : 0u;
      c[u][j] = in && a.col_class ? a.col_class[n] : 0;
      dd[u][j] = d;
      d += 1;
      if (d == D) {
        d = 0;
        n += 1;
        if (n == (uint32_t)a.N) {
          n = 0;
          t += 1;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < FA_U; ++u) {
    const int64_t e0 = e_base + ((int64_t)u * FA_THREADS + threadIdx.x) * 4;
    fl_f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = fa_one(tab, x[u][j], k[u][j], c[u][j], dd[u][j], a.n_classes);
    if (e0 + 4 <= E) {
      *reinterpret_cast<fl_f32x4*>(a.out + e0) = y;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < E) a.out[e0 + j] = y[j];
    }
  }
}

// instantiation (D, keep given) of the two column walks
template <int D>
static void fl_launch_walk(const phx_filter_update_io& io, const bool centred, hipStream_t st) {
  if (io.D == D) {
    const dim3 grid((unsigned)((io.N + FL_LANES - 1) / FL_LANES)), block(FL_LANES);
    if (centred) {
      if (io.keep) hipLaunchKernelGGL((phx_filter_center_kernel<D, true>), grid, block, 0, st, io);
      else hipLaunchKernelGGL((phx_filter_center_kernel<D, false>), grid, block, 0, st, io);
    } else {
      if (io.keep) hipLaunchKernelGGL((phx_filter_sum_kernel<D, true>), grid, block, 0, st, io);
      else hipLaunchKernelGGL((phx_filter_sum_kernel<D, false>), grid, block, 0, st, io);
    }
  } else if constexpr (D > 1) {
    fl_launch_walk<D - 1>(io, centred, st);
  }
}

template <int D>
static void fa_launch(const phx_filter_apply_io& io, const int64_t E, hipStream_t st) {
  if (io.D == D) {
    hipLaunchKernelGGL((phx_filter_apply_kernel<D>), dim3((unsigned)((E + FA_CHUNK - 1) / FA_CHUNK)), dim3(FA_THREADS), 0, st, io, E);
  } else if constexpr (D > 1) {
    fa_launch<D - 1>(io, E, st);
  }
}

// the checks the two calls share; `fn` names the call in the message
static int fl_check(const char* fn, const int T, const int D, const int64_t N, const int n_classes, const void* obs, const void* col_class,
                    const void* state) {
  if (const int rc = frag_rows_cols(fn, T, N)) return rc;
  if (D < 1 || D > FL_MD) return fail(PHX_EINVAL, "%s: D = %d must lie in [1, %d]", fn, D, FL_MD);
  if (n_classes < 1 || n_classes > FL_MC) return fail(PHX_EINVAL, "%s: n_classes = %d must lie in [1, %d]", fn, n_classes, FL_MC);
  if (const int rc = frag_required(fn, obs && state, "obs and state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(obs, state), 16, "obs and state")) return rc;
  return frag_aligned(fn, frag_bits(col_class), 4, "col_class");
}

extern "C" int phx_filter_update(const phx_filter_update_io* io, void* stream) {
  const char* fn = "phx_filter_update";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved, io->reserved0, "the reserved fields")) return rc;
  if (const int rc = fl_check(fn, io->T, io->D, io->N, io->n_classes, io->obs, io->col_class, io->state)) return rc;
  if (!io->workspace || ((uintptr_t)io->workspace & 15u))
    return fail(PHX_EINVAL, "phx_filter_update: workspace is required and must be 16-byte aligned");
  if (io->N > (int64_t)FL_LANES * 0x7fffffff) return frag_beyond_grid(fn, "%lld columns are", (long long)io->N);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned folds = (unsigned)(io->n_classes * io->D);
  FragCall call{fn};
  fl_launch_walk<FL_MD>(*io, false, st);
  if (const int rc = call.launched("the sum", "phx_filter_sum_kernel")) return rc;
  hipLaunchKernelGGL(phx_filter_mean_kernel, dim3(folds), dim3(FL_RED), 0, st, *io);
  if (const int rc = call.launched("the mean", "phx_filter_mean_kernel")) return rc;
  fl_launch_walk<FL_MD>(*io, true, st);
  if (const int rc = call.launched("the centred pass", "phx_filter_center_kernel")) return rc;
  hipLaunchKernelGGL(phx_filter_m2_kernel, dim3(folds), dim3(FL_RED), 0, st, *io);
  if (const int rc = call.launched("the M2 fold", "phx_filter_m2_kernel")) return rc;
  hipLaunchKernelGGL(phx_filter_merge_kernel, dim3(1), dim3(FL_MC * FL_MD), 0, st, *io);
  return call.launched("the merge", "phx_filter_merge_kernel");
}

extern "C" int phx_filter_apply(const phx_filter_apply_io* io, void* stream) {
  const char* fn = "phx_filter_apply";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved, 0, "the reserved fields")) return rc;
  if (const int rc = fl_check(fn, io->T, io->D, io->N, io->n_classes, io->obs, io->col_class, io->state)) return rc;
  if (!io->out || ((uintptr_t)io->out & 15u)) return fail(PHX_EINVAL, "phx_filter_apply: out is required and must be 16-byte aligned");
  if (!(io->clip >= 0.0f)) return fail(PHX_EINVAL, "phx_filter_apply: clip = %g must be >= 0 (0: none)", (double)io->clip);
  // one row's floats and a workgroup's chunk in 32 bits, the chunks in one grid
  if (io->N > (0x7fffffffLL - FA_CHUNK) / io->D || (int64_t)io->T > (0x7fffffffLL * FA_CHUNK) / (io->N * io->D))
    return frag_beyond_grid(fn, "T = %d rows of N = %lld columns are", io->T, (long long)io->N);
  const int64_t E = (int64_t)io->T * io->N * io->D;
  const uintptr_t a = (uintptr_t)io->obs, b = (uintptr_t)io->out, bytes = (uintptr_t)E * 4u;
  if (a != b && a < b + bytes && b < a + bytes)
    return fail(PHX_EINVAL, "phx_filter_apply: out overlaps obs in part (out == obs, exactly in place, is allowed)");
  fa_launch<FL_MD>(*io, E, (hipStream_t)stream);
  return FragCall{fn}.launched(nullptr, "phx_filter_apply_kernel");
}
