// phx_train_batch.hip -- phx_train_batch (include/phantom_amd_batch.h): the kept elements of time-major planes as shuffled RECORDS, one
// column standardized.  Up to four launches on one stream:
//
// phx_batch_count_kernel: a lane owns ONE column and a wave 64 consecutive ones (phx_compact_count_kernel's walk, BC_K rows at a time,
//   rows past the last clamped to it: loaded again, never counted).  It leaves count[n] in start[n] and, with std_plane, the column's
//   two f64 sums in workspace[n] (selects only: an element that is not kept is loaded and dropped).
// phx_batch_scan_kernel: the exclusive i64 prefix over start[0 .. N] in place by one workgroup (phx_compact_scan_kernel's scheme).
// phx_batch_moments_kernel: one 256-thread workgroup folds the per-column sums in the header's fixed order (BM_K pairs loaded ahead of
//   their adds: the fold is a chain of dependent loads otherwise, 37 us against 13 at N = 36 864) and writes `moments`.
// phx_batch_scatter_kernel: a workgroup owns a tile of BT_C consecutive columns and walks T in chunks of BT_R rows: BT_R * BT_C SLOTS.
//   * a record is cut into WINDOWS of 16 words (64 bytes).  A STAGE is one (chunk, window): every slot's 16 words of the window are
//     loaded, a lane on ONE column and a wave-instruction on one (row, word): for a 4-byte plane a coalesced 256-byte row piece, for a
//     w-word plane w such loads over the same lines.  Which plane a word of the record belongs to is a table built once at entry
//     (wave-uniform per load: byte load, word load or a gap's zero); 32 registers per lane;
//   * the NEXT stage's loads are issued before this stage's stores (loads and stores share vmcnt on gfx950),
//     unconditionally: rows past T are clamped to T - 1, columns past the tile's last to it, and after the last stage the same stage
//     is loaded once more -- no global load sits behind a branch of the store phase.  (As compiled today the byte / word / gap branch
//     of the load phase is joined with a full vmcnt wait per word group, which serialises a stage's loads: DESIGN 3.4l);
//   * the registers go to LDS record-major (a slot's 16 words contiguous, the slot stride padded to 20 words), the standardized
//     plane's word as (x - mean) / den;
//   * in a chunk's first stage a lane per column ranks the chunk's kept rows (position p) and every lane then walks the Feistel
//     cycle for two slots (the walk diverges per lane: registers only, no memory operation inside), leaving q per slot in LDS for all
//     windows of the chunk, and stores out_row / out_col;
//   * the store phase: four lanes per slot, each ONE 16-byte LDS read and ONE non-temporal 16-byte store -- a record's window leaves
//     as whole 16-byte stores to 64 consecutive bytes, never one store per plane;
//   * K > capacity is decided from start[N] at entry by every lane alike; the round keys arrive as kernel arguments, mean and den
//     are read once at entry.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_batch.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int BT_R = 8;              // rows per chunk of the scatter (tests/test_gpu_train_batch.py walks T around it)
constexpr int BT_C = 64;             // columns per tile of the scatter: a wave's lanes
constexpr int BT_SB = 4096;          // entries per block of the scan
constexpr int BT_THREADS = 256;      // the scatter's workgroup: four waves
constexpr int BT_WAVES = BT_THREADS / 64;
constexpr int BT_WIN = 16;           // words per window of a record: 64 bytes
constexpr int BT_XW = BT_WIN / BT_WAVES;        // words of a window a wave loads
constexpr int BT_LD = BT_R * BT_XW;             // loads per lane and stage: registers per lane
constexpr int BT_SLOTS = BT_R * BT_C;
constexpr int BT_STRIDE = 20;        // words per slot in LDS (16 + 4: the 16-byte pieces stay aligned)
constexpr int BC_THREADS = 256;      // the count's workgroup
constexpr int BC_K = 8;              // rows per chunk of the count
constexpr int BM_K = 8;              // pairs a lane of the moments kernel loads ahead of its adds
constexpr int BS_THREADS = 1024;     // the scan's workgroup
constexpr int BS_ITEMS = BT_SB / BS_THREADS;
constexpr int BM_THREADS = 256;      // the moments' workgroup: the header's 256 lane values
constexpr uint32_t BT_GAP = 0xffffu; // a word of the record that no plane covers

typedef uint32_t bt_u32x4 __attribute__((ext_vector_type(4)));

struct BtKeys {
  uint32_t key[6];
};

__global__ __launch_bounds__(BC_THREADS) void phx_batch_count_kernel(const uint8_t* __restrict__ keep, const uint8_t* __restrict__ col_class,
                                                                     const float* __restrict__ x, int64_t* __restrict__ start,
                                                                     double* __restrict__ sums, const int T, const int64_t N, const int S,
                                                                     const int class_id) {
  const int64_t n = (int64_t)blockIdx.x * BC_THREADS + threadIdx.x;
  if (n >= N) return;
  const bool in_class = col_class == nullptr || col_class[n % S] == class_id;
  uint32_t cnt = 0;
  double s = 0.0, q = 0.0;
  for (int t0 = 0; t0 < T; t0 += BC_K) {
    uint32_t kp[BC_K];
    float v[BC_K];
#pragma unroll
    for (int k = 0; k < BC_K; ++k) {
      const int t = t0 + k < T ? t0 + k : T - 1;
      kp[k] = keep ? keep[(int64_t)t * N + n] : 1u;                        // (uniform)
      v[k] = x ? x[(int64_t)t * N + n] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < BC_K; ++k) {
      const bool kept = t0 + k < T && kp[k] != 0 && in_class;
      const double d = (double)v[k];
      cnt += kept ? 1u : 0u;
      s = kept ? s + d : s;
      q = kept ? q + d * d : q;
    }
  }
  start[n] = (int64_t)cnt;
  if (x) {
    sums[2 * n] = s;
    sums[2 * n + 1] = q;
  }
}

// entries [i0, i0 + BT_SB) of the counts, BS_ITEMS consecutive ones per thread; entry N and beyond: 0 (start[N] holds no count)
__device__ __forceinline__ void bs_load(int64_t (&v)[BS_ITEMS], const int64_t* start, const int64_t i0, const int64_t N) {
#pragma unroll
  for (int e = 0; e < BS_ITEMS; ++e) {
    const int64_t i = i0 + (int64_t)threadIdx.x * BS_ITEMS + e;
    v[e] = i < N ? start[i] : 0;
  }
}

__global__ __launch_bounds__(BS_THREADS) void phx_batch_scan_kernel(int64_t* start, const int64_t N) {
  __shared__ int64_t wsum[BS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  int64_t v[BS_ITEMS], nx[BS_ITEMS];
  bs_load(v, start, 0, N);
  for (int64_t i0 = 0; i0 <= N; i0 += BT_SB) {
    bs_load(nx, start, i0 + BT_SB, N);                                     // (the next block's loads before this block's stores)
    int64_t s = 0;
#pragma unroll
    for (int e = 0; e < BS_ITEMS; ++e) s += v[e];
    int64_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d);
      inc += lane >= d ? up : 0;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < BS_THREADS / 64; ++j) {
      const int64_t x = wsum[j];
      before += j < wave ? x : 0;
      total += x;
    }
    int64_t ex = carry + before + inc - s;
#pragma unroll
    for (int e = 0; e < BS_ITEMS; ++e) {
      const int64_t i = i0 + (int64_t)threadIdx.x * BS_ITEMS + e;
      if (i <= N) start[i] = ex;
      ex += v[e];
    }
    carry += total;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < BS_ITEMS; ++e) v[e] = nx[e];
  }
}

__global__ __launch_bounds__(BM_THREADS) void phx_batch_moments_kernel(const double* __restrict__ sums, const int64_t* __restrict__ start,
                                                                       phx_batch_moments* __restrict__ moments, const int64_t N) {
  __shared__ double ls[BM_THREADS], lq[BM_THREADS];
  const int i = (int)threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int64_t j0 = i; j0 < N; j0 += (int64_t)BM_K * BM_THREADS) {       // (BM_K loads in flight; the adds in the header's order)
    double a[BM_K], b[BM_K];
#pragma unroll
    for (int k = 0; k < BM_K; ++k) {
      const int64_t j = j0 + (int64_t)k * BM_THREADS;
      const int64_t jc = j < N ? j : N - 1;
      a[k] = sums[2 * jc];
      b[k] = sums[2 * jc + 1];
    }
#pragma unroll
    for (int k = 0; k < BM_K; ++k) {
      const bool in = j0 + (int64_t)k * BM_THREADS < N;
      s = in ? s + a[k] : s;
      q = in ? q + b[k] : q;
    }
  }
  ls[i] = s;
  lq[i] = q;
  __syncthreads();
  for (int h = BM_THREADS / 2; h >= 1; h >>= 1) {
    if (i < h) {
      s = s + ls[i + h];
      q = q + lq[i + h];
      ls[i] = s;
      lq[i] = q;
    }
    __syncthreads();
  }
  if (i == 0) {
    const int64_t K = start[N];
    phx_batch_moments m;
    m.count = K;
    m.sum = s;
    m.sumsq = q;
    m.mean = 0.0f;
    m.den = 1e-4f;
    if (K > 0) {
      const double mu = s / (double)K;
      double v = q / (double)K - mu * mu;
      v = v > 0.0 ? v : 0.0;
      const float sd = (float)__builtin_sqrt(v);
      m.mean = (float)mu;
      m.den = sd > 1e-4f ? sd : 1e-4f;
    }
    *moments = m;
  }
}

// the header's round function and walk: registers only
__device__ __forceinline__ uint32_t bt_round(const uint32_t R, const uint32_t key, const uint32_t mask) {
  uint32_t x = R ^ key;
  x *= 0x9E3779B1u; x ^= x >> 15;
  x *= 0x85EBCA77u; x ^= x >> 13;
  x *= 0xC2B2AE3Du; x ^= x >> 16;
  return x & mask;
}

__device__ __forceinline__ int64_t bt_perm(const int64_t p, const int64_t K, const int h, const uint32_t mask, const BtKeys& keys) {
  uint64_t x = (uint64_t)p;
  do {
    uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t nr = L ^ bt_round(R, keys.key[r], mask);
      L = R;
      R = nr;
    }
    x = ((uint64_t)L << h) | R;
  } while (x >= (uint64_t)K);
  return (int64_t)x;
}

struct BtTile {
  uint32_t rec[BT_SLOTS * BT_STRIDE];          // [slot][word of the window]: slot = row of the chunk * BT_C + column of the tile
  int64_t q[BT_SLOTS];                         // the slot's record, -1: not kept (per chunk, for every window of it)
  int64_t base[BT_C];                          // the position of the column's next kept element
  uint32_t wmap[256];                          // per word of the record: plane | word of the element << 8, or BT_GAP
  uint8_t keep[BT_SLOTS];                      // the chunk's keep bytes
  uint8_t in_class[BT_C];
};

// one stage's loads: word x = win * 16 + wave * 4 + xi of rows t0 .. t0 + BT_R - 1 in v[r * BT_XW + xi], this lane's column
__device__ __forceinline__ void bt_load(uint32_t (&v)[BT_LD], uint32_t (&kp)[BT_SLOTS / BT_THREADS], const phx_train_batch_io& a, const BtTile& s,
                                        const int t0, const int win, const int64_t n0, const int ncol, const int lane, const int wave) {
  const int T = (int)a.T;
  const int64_t n = n0 + (lane < ncol ? lane : ncol - 1);
#pragma unroll
  for (int xi = 0; xi < BT_XW; ++xi) {
    const int x = win * BT_WIN + wave * BT_XW + xi;
    const uint32_t m = __builtin_amdgcn_readfirstlane(x < a.row_words ? s.wmap[x] : BT_GAP);
    if (m == BT_GAP) {                                                     // (wave-uniform; the load phase)
#pragma unroll
      for (int r = 0; r < BT_R; ++r) v[r * BT_XW + xi] = 0u;
    } else {
      const int k = (int)(m & 0xffu), j = (int)(m >> 8);
      const int eb = a.plane[k].elem_bytes;
      if (eb == 1) {
        const uint8_t* src = static_cast<const uint8_t*>(a.plane[k].src) + n;
#pragma unroll
        for (int r = 0; r < BT_R; ++r) {
          const int t = t0 + r < T ? t0 + r : T - 1;
          v[r * BT_XW + xi] = src[(int64_t)t * a.N];
        }
      } else {
        const int w = eb >> 2;
        const uint32_t* src = static_cast<const uint32_t*>(a.plane[k].src) + (n * w + j);
        const int64_t pitch = a.N * w;
#pragma unroll
        for (int r = 0; r < BT_R; ++r) {
          const int t = t0 + r < T ? t0 + r : T - 1;
          v[r * BT_XW + xi] = src[(int64_t)t * pitch];
        }
      }
    }
  }
  // the chunk's keep bytes: slot = i * 256 + thread
#pragma unroll
  for (int i = 0; i < BT_SLOTS / BT_THREADS; ++i) {
    const int slot = i * BT_THREADS + wave * 64 + lane;
    const int r = slot / BT_C;
    const int t = t0 + r < T ? t0 + r : T - 1;
    kp[i] = a.keep ? a.keep[(int64_t)t * a.N + n] : 1u;                    // (uniform; slot % BT_C == lane)
  }
}

__global__ __launch_bounds__(BT_THREADS) void phx_batch_scatter_kernel(const phx_train_batch_io a, const BtKeys keys) {
  __shared__ __attribute__((aligned(16))) BtTile s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = (int)a.T;
  const int64_t K = a.start[a.N];
  if (K > a.capacity) return;                                              // (every lane of the grid alike)
  const int64_t n0 = (int64_t)blockIdx.x * BT_C;
  const int ncol = (int)(a.N - n0 < BT_C ? a.N - n0 : BT_C);
  const int n_win = (a.row_words + BT_WIN - 1) / BT_WIN;
  // w: the smallest even integer >= 2 with 2^w >= K
  const bool shuffled = a.shuffle != 0 && K > 1;
  const int bits = K > 1 ? 64 - __clzll((unsigned long long)(K - 1)) : 0;
  const int wbits = bits < 2 ? 2 : bits + (bits & 1);
  const int h = wbits >> 1;
  const uint32_t mask = (uint32_t)((1ull << h) - 1ull);
  const bool has_std = a.std_plane >= 0;
  float mean = 0.0f, den = 1.0f;
  if (has_std) {                                                           // (uniform; read once)
    mean = a.moments->mean;
    den = a.moments->den;
  }
  if (threadIdx.x < BT_C) {
    const bool in = (int)threadIdx.x < ncol;
    const int64_t n = n0 + (in ? threadIdx.x : 0);
    s.base[threadIdx.x] = in ? a.start[n] : 0;
    s.in_class[threadIdx.x] = in && (a.col_class == nullptr || a.col_class[n % a.S] == a.class_id) ? 1 : 0;
  }
  {                                                                        // the plane and element word of every word of a record
    const int x = (int)threadIdx.x;
    uint32_t m = BT_GAP;
    for (int k = 0; k < a.n_planes; ++k) {
      const int eb = a.plane[k].elem_bytes, off = a.plane[k].word_off;
      const int w = eb == 1 ? 1 : eb >> 2;
      if (x >= off && x < off + w) m = (uint32_t)k | ((uint32_t)(x - off) << 8);
    }
    s.wmap[x] = m;
  }
  __syncthreads();
  const uint32_t std_word = has_std ? (uint32_t)a.plane[a.std_plane].word_off : 0xffffffffu;
  int t0 = 0, win = 0;
  uint32_t v[BT_LD], kp[BT_SLOTS / BT_THREADS];
  bt_load(v, kp, a, s, t0, win, n0, ncol, lane, wave);
  for (;;) {
    // registers to LDS, record-major
#pragma unroll
    for (int xi = 0; xi < BT_XW; ++xi) {
      const int xl = wave * BT_XW + xi;
      const bool is_std = (uint32_t)(win * BT_WIN + xl) == std_word;       // (wave-uniform)
#pragma unroll
      for (int r = 0; r < BT_R; ++r) {
        uint32_t u = v[r * BT_XW + xi];
        if (is_std) u = __float_as_uint((__uint_as_float(u) - mean) / den);
        s.rec[(r * BT_C + lane) * BT_STRIDE + xl] = u;
      }
    }
    if (win == 0) {
#pragma unroll
      for (int i = 0; i < BT_SLOTS / BT_THREADS; ++i) s.keep[i * BT_THREADS + threadIdx.x] = (uint8_t)(kp[i] != 0);
    }
    __syncthreads();
    int nt0 = t0, nwin = win + 1;
    if (nwin == n_win) {
      nwin = 0;
      nt0 = t0 + BT_R;
    }
    const bool more = nt0 < T;
    bt_load(v, kp, a, s, more ? nt0 : t0, more ? nwin : win, n0, ncol, lane, wave);      // (after the last stage: the same one again, never used)
    if (win == 0) {                                                        // the chunk's positions and records
      if (threadIdx.x < BT_C) {
        const int c = (int)threadIdx.x;
        int64_t p = s.base[c];
        const bool in = s.in_class[c] != 0;
#pragma unroll
        for (int r = 0; r < BT_R; ++r) {
          const bool kept = in && t0 + r < T && s.keep[r * BT_C + c] != 0;
          s.q[r * BT_C + c] = kept ? p : -1;
          p += kept ? 1 : 0;
        }
        s.base[c] = p;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < BT_SLOTS / BT_THREADS; ++i) {
        const int slot = i * BT_THREADS + (int)threadIdx.x;
        const int64_t p = s.q[slot];
        if (p >= 0) {
          const int64_t q = shuffled ? bt_perm(p, K, h, mask, keys) : p;
          s.q[slot] = q;
          if (a.out_row) __builtin_nontemporal_store((int32_t)(t0 + slot / BT_C), a.out_row + q);
          if (a.out_col) __builtin_nontemporal_store((int32_t)(n0 + slot % BT_C), a.out_col + q);
        }
      }
      __syncthreads();
    }
    if (a.records) {                                                       // four lanes per slot: one 16-byte piece each
      const int pieces = (a.row_words - win * BT_WIN) >> 2;                // (of this window; row_words is a multiple of 4)
      const int piece = (int)threadIdx.x & 3;
#pragma unroll
      for (int i = 0; i < BT_SLOTS * 4 / BT_THREADS; ++i) {
        const int slot = i * (BT_THREADS / 4) + ((int)threadIdx.x >> 2);
        const int64_t q = s.q[slot];
        const bt_u32x4 u = *reinterpret_cast<const bt_u32x4*>(&s.rec[slot * BT_STRIDE + piece * 4]);
        if (q >= 0 && piece < pieces)
          __builtin_nontemporal_store(u, reinterpret_cast<bt_u32x4*>(a.records + (q * a.row_words + win * BT_WIN + piece * 4)));
      }
    }
    __syncthreads();
    if (!more) break;
    t0 = nt0;
    win = nwin;
  }
}

extern "C" int phx_train_batch(const phx_train_batch_io* io, void* stream) {
  const char* fn = "phx_train_batch";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_batch_shape(fn, *io, BT_C)) return rc;
  if (const int rc = frag_batch_record(fn, *io, PHX_BATCH_MAX_PLANES)) return rc;
  if (const int rc = frag_batch_buffers(fn, *io, io->start, "start")) return rc;
  if (io->out_col && io->N > 0x7fffffffLL) return fail(PHX_EINVAL, "phx_train_batch: out_col needs N = %lld <= 2^31 - 1", (long long)io->N);
  if (const int rc = frag_batch_planes(fn, *io)) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->start, io->records, io->out_row, io->out_col, io->moments, io->workspace), 16,
                                  "start, records, out_row, out_col, moments and workspace"))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  const bool has_std = io->std_plane >= 0;
  const float* x = has_std ? static_cast<const float*>(io->plane[io->std_plane].src) : nullptr;
  hipLaunchKernelGGL(phx_batch_count_kernel, dim3((unsigned)((io->N + BC_THREADS - 1) / BC_THREADS)), dim3(BC_THREADS), 0, st, io->keep, io->col_class,
                     x, io->start, static_cast<double*>(io->workspace), (int)io->T, io->N, io->S, io->class_id);
  if (const int rc = call.launched("the count", "phx_batch_count_kernel")) return rc;
  hipLaunchKernelGGL(phx_batch_scan_kernel, dim3(1), dim3(BS_THREADS), 0, st, io->start, io->N);
  if (const int rc = call.launched("the scan", "phx_batch_scan_kernel")) return rc;
  if (has_std) {
    hipLaunchKernelGGL(phx_batch_moments_kernel, dim3(1), dim3(BM_THREADS), 0, st, static_cast<const double*>(io->workspace), io->start, io->moments,
                       io->N);
    if (const int rc = call.launched("the moments", "phx_batch_moments_kernel")) return rc;
  }
  if (io->capacity == 0 || (!io->records && !io->out_row && !io->out_col)) return PHX_OK;      // (nothing to write)
  BtKeys keys;
  frag_round_keys(io->seed, io->epoch, keys.key);
  hipLaunchKernelGGL(phx_batch_scatter_kernel, dim3((unsigned)((io->N + BT_C - 1) / BT_C)), dim3(BT_THREADS), 0, st, *io, keys);
  return call.launched("the scatter", "phx_batch_scatter_kernel");
}
