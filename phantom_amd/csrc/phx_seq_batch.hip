// phx_seq_batch.hip -- phx_seq_batch (include/phantom_amd_seq.h): every column's kept rows cut into sequences of at most L rows, padded
// to L with zeros, the sequences shuffled, one column standardized.  Up to four launches on one stream.  The scan, the
// fold and the Feistel walk are COPIES of phx_train_batch.hip's (sharing the bodies through a header changed the older
// kernels' register allocation), under names of their own.
//
// phx_seq_count_kernel: a lane owns ONE column and walks T, SC_K rows at a time (rows past the last clamped to it: loaded again, never
//   counted), carrying the open sequence's length.  It leaves Q_n in seq_start[n] and, with std_plane, the column's two f64 sums and its
//   kept rows in workspace (selects only: an element that is not kept is loaded and dropped, its flags with it).
// phx_seq_scan_kernel: the exclusive i64 prefix over seq_start[0 .. N] in place by one workgroup.
// phx_seq_moments_kernel: one 256-thread workgroup folds the per-column sums in the header's fixed order, adds up the kept rows (K is
//   not seq_start[N] here) and writes `moments`.
// phx_seq_scatter_kernel: phx_batch_scatter_kernel's stages -- a workgroup owns a tile of SQ_C consecutive columns and walks T in chunks
//   of SQ_R rows; a record is cut into windows of 16 words; the next stage's loads are issued before this stage's stores; records are
//   staged in LDS record-major and leave as whole 16-byte non-temporal stores -- with these differences:
//   * in a chunk's first stage the lane of a column walks the chunk's rows with the column's carried (sequence index, len, first_row),
//     held in that lane's registers across chunks, and leaves per slot the sequence index, the position i and -- where the row closes
//     its sequence -- first_row;
//   * every lane then walks the Feistel cycle of its slots' SEQUENCE index (Q in the place of K), turns it into the slot
//     sigma * L + i, stores out_row / out_col, and for a closing row stores seq_lens / seq_row / seq_col and, where seq_len < L, appends
//     its slot to a list in LDS;
//   * after the chunk's record stores the workgroup zero-fills the listed padding, a wave per entry, in 16-byte non-temporal stores,
//     and writes -1 into out_row / out_col there: the padding is written where its sequence closes, by the workgroup that knows
//     seq_len, and no fifth kernel reads seq_lens back;
//   * after the last chunk the column lanes close what is still open, and the list is served once more.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_seq.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int SQ_R = 8;              // rows per chunk of the scatter (tests/test_gpu_seq_batch.py walks T and L around it)
constexpr int SQ_C = 64;             // columns per tile of the scatter: a wave's lanes
constexpr int SQ_SB = 4096;          // entries per block of the scan
constexpr int SQ_THREADS = 256;      // the scatter's workgroup: four waves
constexpr int SQ_WAVES = SQ_THREADS / 64;
constexpr int SQ_WIN = 16;           // words per window of a record: 64 bytes
constexpr int SQ_XW = SQ_WIN / SQ_WAVES;        // words of a window a wave loads
constexpr int SQ_LD = SQ_R * SQ_XW;             // loads per lane and stage: registers per lane
constexpr int SQ_SLOTS = SQ_R * SQ_C;
constexpr int SQ_PER = SQ_SLOTS / SQ_THREADS;   // slots per thread
constexpr int SQ_STRIDE = 20;        // words per slot in LDS (16 + 4: the 16-byte pieces stay aligned)
constexpr int SC_THREADS = 256;      // the count's workgroup
constexpr int SC_K = 8;              // rows per chunk of the count
constexpr int SM_K = 8;              // triples a lane of the moments kernel loads ahead of its adds
constexpr int SS_THREADS = 1024;     // the scan's workgroup
constexpr int SS_ITEMS = SQ_SB / SS_THREADS;
constexpr int SM_THREADS = 256;      // the moments' workgroup: the header's 256 lane values
constexpr uint32_t SQ_GAP = 0xffffu; // a word of the record that no plane covers

typedef uint32_t sq_u32x4 __attribute__((ext_vector_type(4)));

struct SqKeys {
  uint32_t key[6];
};

__global__ __launch_bounds__(SC_THREADS) void phx_seq_count_kernel(const uint8_t* __restrict__ keep, const uint8_t* __restrict__ col_class,
                                                                   const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                   const float* __restrict__ x, int64_t* __restrict__ seq_start,
                                                                   double* __restrict__ sums, int64_t* __restrict__ rows, const int T,
                                                                   const int64_t N, const int S, const int class_id, const int L) {
  const int64_t n = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (n >= N) return;
  const bool in_class = col_class == nullptr || col_class[n % S] == class_id;
  uint32_t cnt = 0, nseq = 0;
  int len = 0;
  double s = 0.0, q = 0.0;
  for (int t0 = 0; t0 < T; t0 += SC_K) {
    uint32_t kp[SC_K], fl[SC_K];
    float v[SC_K];
#pragma unroll
    for (int k = 0; k < SC_K; ++k) {
      const int t = t0 + k < T ? t0 + k : T - 1;
      kp[k] = keep ? keep[(int64_t)t * N + n] : 1u;                        // (uniform)
      fl[k] = (term ? term[(int64_t)t * N + n] : 0u) | (trunc ? trunc[(int64_t)t * N + n] : 0u);
      v[k] = x ? x[(int64_t)t * N + n] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < SC_K; ++k) {
      const bool kept = t0 + k < T && kp[k] != 0 && in_class;
      const double d = (double)v[k];
      cnt += kept ? 1u : 0u;
      s = kept ? s + d : s;
      q = kept ? q + d * d : q;
      len += kept ? 1 : 0;
      const bool closes = kept && (fl[k] != 0 || len == L);
      nseq += closes ? 1u : 0u;
      len = closes ? 0 : len;
    }
  }
  seq_start[n] = (int64_t)nseq + (len > 0 ? 1 : 0);
  if (x) {
    sums[2 * n] = s;
    sums[2 * n + 1] = q;
    rows[n] = (int64_t)cnt;
  }
}

// entries [i0, i0 + SQ_SB) of the counts, SS_ITEMS consecutive ones per thread; entry N and beyond: 0 (seq_start[N] holds no count)
__device__ __forceinline__ void ss_load(int64_t (&v)[SS_ITEMS], const int64_t* start, const int64_t i0, const int64_t N) {
#pragma unroll
  for (int e = 0; e < SS_ITEMS; ++e) {
    const int64_t i = i0 + (int64_t)threadIdx.x * SS_ITEMS + e;
    v[e] = i < N ? start[i] : 0;
  }
}

__global__ __launch_bounds__(SS_THREADS) void phx_seq_scan_kernel(int64_t* start, const int64_t N) {
  __shared__ int64_t wsum[SS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  int64_t v[SS_ITEMS], nx[SS_ITEMS];
  ss_load(v, start, 0, N);
  for (int64_t i0 = 0; i0 <= N; i0 += SQ_SB) {
    ss_load(nx, start, i0 + SQ_SB, N);                                     // (the next block's loads before this block's stores)
    int64_t s = 0;
#pragma unroll
    for (int e = 0; e < SS_ITEMS; ++e) s += v[e];
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
    for (int j = 0; j < SS_THREADS / 64; ++j) {
      const int64_t x = wsum[j];
      before += j < wave ? x : 0;
      total += x;
    }
    int64_t ex = carry + before + inc - s;
#pragma unroll
    for (int e = 0; e < SS_ITEMS; ++e) {
      const int64_t i = i0 + (int64_t)threadIdx.x * SS_ITEMS + e;
      if (i <= N) start[i] = ex;
      ex += v[e];
    }
    carry += total;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < SS_ITEMS; ++e) v[e] = nx[e];
  }
}

__global__ __launch_bounds__(SM_THREADS) void phx_seq_moments_kernel(const double* __restrict__ sums, const int64_t* __restrict__ rows,
                                                                     phx_batch_moments* __restrict__ moments, const int64_t N) {
  __shared__ double ls[SM_THREADS], lq[SM_THREADS];
  __shared__ int64_t lk[SM_THREADS];
  const int i = (int)threadIdx.x;
  double s = 0.0, q = 0.0;
  int64_t kept = 0;
  for (int64_t j0 = i; j0 < N; j0 += (int64_t)SM_K * SM_THREADS) {       // (SM_K loads in flight; the adds in the header's order)
    double a[SM_K], b[SM_K];
    int64_t c[SM_K];
#pragma unroll
    for (int k = 0; k < SM_K; ++k) {
      const int64_t j = j0 + (int64_t)k * SM_THREADS;
      const int64_t jc = j < N ? j : N - 1;
      a[k] = sums[2 * jc];
      b[k] = sums[2 * jc + 1];
      c[k] = rows[jc];
    }
#pragma unroll
    for (int k = 0; k < SM_K; ++k) {
      const bool in = j0 + (int64_t)k * SM_THREADS < N;
      s = in ? s + a[k] : s;
      q = in ? q + b[k] : q;
      kept += in ? c[k] : 0;
    }
  }
  ls[i] = s;
  lq[i] = q;
  lk[i] = kept;
  __syncthreads();
  for (int h = SM_THREADS / 2; h >= 1; h >>= 1) {
    if (i < h) {
      s = s + ls[i + h];
      q = q + lq[i + h];
      kept += lk[i + h];
      ls[i] = s;
      lq[i] = q;
      lk[i] = kept;
    }
    __syncthreads();
  }
  if (i == 0) {
    const int64_t K = kept;
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

// phantom_amd_batch.h's round function and walk: registers only
__device__ __forceinline__ uint32_t sq_round(const uint32_t R, const uint32_t key, const uint32_t mask) {
  uint32_t x = R ^ key;
  x *= 0x9E3779B1u; x ^= x >> 15;
  x *= 0x85EBCA77u; x ^= x >> 13;
  x *= 0xC2B2AE3Du; x ^= x >> 16;
  return x & mask;
}

__device__ __forceinline__ int64_t sq_perm(const int64_t p, const int64_t K, const int h, const uint32_t mask, const SqKeys& keys) {
  uint64_t x = (uint64_t)p;
  do {
    uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t nr = L ^ sq_round(R, keys.key[r], mask);
      L = R;
      R = nr;
    }
    x = ((uint64_t)L << h) | R;
  } while (x >= (uint64_t)K);
  return (int64_t)x;
}

struct SqTile {
  uint32_t rec[SQ_SLOTS * SQ_STRIDE];          // [slot][word of the window]: slot = row of the chunk * SQ_C + column of the tile
  int64_t q[SQ_SLOTS];                         // the slot's sequence index, then its output slot; -1: not kept (per chunk)
  int32_t pos[SQ_SLOTS];                       // the slot's position i in its sequence
  int32_t first[SQ_SLOTS];                     // first_row where the slot closes its sequence, else -1
  uint32_t wmap[256];                          // per word of the record: plane | word of the element << 8, or SQ_GAP
  uint8_t keep[SQ_SLOTS];                      // the chunk's bytes: bit 0 keep != 0, bit 1 terminated | truncated != 0
  uint8_t in_class[SQ_C];
  uint16_t pad_idx[SQ_SLOTS];                  // the padding list: the slots of the chunk whose row closed a sequence short of L
  int32_t pad_n;                               // entries of the padding list
};

// one stage's loads: word x = win * 16 + wave * 4 + xi of rows t0 .. t0 + SQ_R - 1 in v[r * SQ_XW + xi], this lane's column
__device__ __forceinline__ void sq_load(uint32_t (&v)[SQ_LD], uint32_t (&kp)[SQ_PER], const phx_seq_batch_io& a, const SqTile& s, const int t0,
                                        const int win, const int64_t n0, const int ncol, const int lane, const int wave) {
  const int T = (int)a.T;
  const int64_t n = n0 + (lane < ncol ? lane : ncol - 1);
#pragma unroll
  for (int xi = 0; xi < SQ_XW; ++xi) {
    const int x = win * SQ_WIN + wave * SQ_XW + xi;
    const uint32_t m = __builtin_amdgcn_readfirstlane(x < a.row_words ? s.wmap[x] : SQ_GAP);
    if (m == SQ_GAP) {                                                     // (wave-uniform; the load phase)
#pragma unroll
      for (int r = 0; r < SQ_R; ++r) v[r * SQ_XW + xi] = 0u;
    } else {
      const int k = (int)(m & 0xffu), j = (int)(m >> 8);
      const int eb = a.plane[k].elem_bytes;
      if (eb == 1) {
        const uint8_t* src = static_cast<const uint8_t*>(a.plane[k].src) + n;
#pragma unroll
        for (int r = 0; r < SQ_R; ++r) {
          const int t = t0 + r < T ? t0 + r : T - 1;
          v[r * SQ_XW + xi] = src[(int64_t)t * a.N];
        }
      } else {
        const int w = eb >> 2;
        const uint32_t* src = static_cast<const uint32_t*>(a.plane[k].src) + (n * w + j);
        const int64_t pitch = a.N * w;
#pragma unroll
        for (int r = 0; r < SQ_R; ++r) {
          const int t = t0 + r < T ? t0 + r : T - 1;
          v[r * SQ_XW + xi] = src[(int64_t)t * pitch];
        }
      }
    }
  }
  // the chunk's keep and flag bytes: slot = i * 256 + thread
#pragma unroll
  for (int i = 0; i < SQ_PER; ++i) {
    const int slot = i * SQ_THREADS + wave * 64 + lane;
    const int r = slot / SQ_C;
    const int t = t0 + r < T ? t0 + r : T - 1;
    const int64_t e = (int64_t)t * a.N + n;                                // (slot % SQ_C == lane)
    const uint32_t k = a.keep ? a.keep[e] : 1u;                            // (uniform)
    const uint32_t f = (a.terminated ? a.terminated[e] : 0u) | (a.truncated ? a.truncated[e] : 0u);
    kp[i] = (k != 0 ? 1u : 0u) | (f != 0 ? 2u : 0u);
  }
}

// a sequence closes at the row of `slot` (s.q[slot] and s.pos[slot] hold its output slot and position): its three outputs, and its
// padding onto the list
__device__ __forceinline__ void sq_close(const phx_seq_batch_io& a, SqTile& s, const int slot, const int64_t sigma, const int len, const int first,
                                         const int64_t n) {
  const int L = (int)a.max_seq_len;
  if (a.seq_lens) __builtin_nontemporal_store((int32_t)len, a.seq_lens + sigma);
  if (a.seq_row) __builtin_nontemporal_store((int32_t)first, a.seq_row + sigma);
  if (a.seq_col) __builtin_nontemporal_store((int32_t)n, a.seq_col + sigma);
  if (len < L) {
    const int e = atomicAdd(&s.pad_n, 1);                                  // (at most one entry per slot of a chunk: e < SQ_SLOTS)
    s.pad_idx[e] = (uint16_t)slot;
  }
}

// the listed padding: a wave per entry, zeros in 16-byte pieces and -1 in out_row / out_col.  The list is complete (a barrier behind
// its last append) and stays as it is until the barrier behind this
__device__ __forceinline__ void sq_pad(const phx_seq_batch_io& a, const SqTile& s, const int lane, const int wave) {
  const int n = s.pad_n;
  const sq_u32x4 zero = {0u, 0u, 0u, 0u};
  for (int e = wave; e < n; e += SQ_WAVES) {
    const int idx = s.pad_idx[e];
    const int64_t slot0 = s.q[idx] + 1;                                    // (behind the sequence's last row)
    const int cnt = (int)a.max_seq_len - 1 - s.pos[idx];
    if (a.records) {
      const int64_t pieces = (int64_t)cnt * (a.row_words >> 2);
      sq_u32x4* dst = reinterpret_cast<sq_u32x4*>(a.records + slot0 * a.row_words);
      for (int64_t p = lane; p < pieces; p += 64) __builtin_nontemporal_store(zero, dst + p);
    }
    for (int i = lane; i < cnt; i += 64) {
      if (a.out_row) __builtin_nontemporal_store((int32_t)-1, a.out_row + slot0 + i);
      if (a.out_col) __builtin_nontemporal_store((int32_t)-1, a.out_col + slot0 + i);
    }
  }
}

__global__ __launch_bounds__(SQ_THREADS) void phx_seq_scatter_kernel(const phx_seq_batch_io a, const SqKeys keys) {
  __shared__ __attribute__((aligned(16))) SqTile s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = (int)a.T;
  const int L = (int)a.max_seq_len;
  const int64_t Q = a.seq_start[a.N];
  if (Q > a.capacity) return;                                              // (every lane of the grid alike)
  const int64_t n0 = (int64_t)blockIdx.x * SQ_C;
  const int ncol = (int)(a.N - n0 < SQ_C ? a.N - n0 : SQ_C);
  const int n_win = (a.row_words + SQ_WIN - 1) / SQ_WIN;
  // w: the smallest even integer >= 2 with 2^w >= Q
  const bool shuffled = a.shuffle != 0 && Q > 1;
  const int bits = Q > 1 ? 64 - __clzll((unsigned long long)(Q - 1)) : 0;
  const int wbits = bits < 2 ? 2 : bits + (bits & 1);
  const int h = wbits >> 1;
  const uint32_t mask = (uint32_t)((1ull << h) - 1ull);
  const bool has_std = a.std_plane >= 0;
  float mean = 0.0f, den = 1.0f;
  if (has_std) {                                                           // (uniform; read once)
    mean = a.moments->mean;
    den = a.moments->den;
  }
  // the column's walk, carried across chunks in the registers of the column's lane (threads below SQ_C)
  int64_t seq = 0;                                                         // the index of the column's open (or next) sequence
  int len = 0, first = 0;
  if (threadIdx.x < SQ_C) {
    const bool in = (int)threadIdx.x < ncol;
    const int64_t n = n0 + (in ? threadIdx.x : 0);
    seq = in ? a.seq_start[n] : 0;
    s.in_class[threadIdx.x] = in && (a.col_class == nullptr || a.col_class[n % a.S] == a.class_id) ? 1 : 0;
  }
  {                                                                        // the plane and element word of every word of a record
    const int x = (int)threadIdx.x;
    uint32_t m = SQ_GAP;
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
  uint32_t v[SQ_LD], kp[SQ_PER];
  sq_load(v, kp, a, s, t0, win, n0, ncol, lane, wave);
  for (;;) {
    // registers to LDS, record-major
#pragma unroll
    for (int xi = 0; xi < SQ_XW; ++xi) {
      const int xl = wave * SQ_XW + xi;
      const bool is_std = (uint32_t)(win * SQ_WIN + xl) == std_word;       // (wave-uniform)
#pragma unroll
      for (int r = 0; r < SQ_R; ++r) {
        uint32_t u = v[r * SQ_XW + xi];
        if (is_std) u = __float_as_uint((__uint_as_float(u) - mean) / den);
        s.rec[(r * SQ_C + lane) * SQ_STRIDE + xl] = u;
      }
    }
    if (win == 0) {
#pragma unroll
      for (int i = 0; i < SQ_PER; ++i) s.keep[i * SQ_THREADS + threadIdx.x] = (uint8_t)kp[i];
      if (threadIdx.x == 0) s.pad_n = 0;
    }
    __syncthreads();
    int nt0 = t0, nwin = win + 1;
    if (nwin == n_win) {
      nwin = 0;
      nt0 = t0 + SQ_R;
    }
    const bool more = nt0 < T;
    sq_load(v, kp, a, s, more ? nt0 : t0, more ? nwin : win, n0, ncol, lane, wave);      // (after the last stage: the same one again, never used)
    if (win == 0) {                                                        // the chunk's sequences, positions and slots
      if (threadIdx.x < SQ_C) {
        const int c = (int)threadIdx.x;
        const bool in = s.in_class[c] != 0;
#pragma unroll
        for (int r = 0; r < SQ_R; ++r) {
          const uint32_t b = s.keep[r * SQ_C + c];
          const bool kept = in && t0 + r < T && (b & 1u) != 0;
          first = kept && len == 0 ? t0 + r : first;
          s.q[r * SQ_C + c] = kept ? seq : -1;
          s.pos[r * SQ_C + c] = len;
          len += kept ? 1 : 0;
          const bool closes = kept && ((b & 2u) != 0 || len == L);
          s.first[r * SQ_C + c] = closes ? first : -1;
          seq += closes ? 1 : 0;
          len = closes ? 0 : len;
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < SQ_PER; ++i) {
        const int slot = i * SQ_THREADS + (int)threadIdx.x;
        const int64_t p = s.q[slot];
        if (p >= 0) {
          const int64_t sigma = shuffled ? sq_perm(p, Q, h, mask, keys) : p;
          const int pos = s.pos[slot];
          const int64_t q = sigma * L + pos;
          s.q[slot] = q;
          if (a.out_row) __builtin_nontemporal_store((int32_t)(t0 + slot / SQ_C), a.out_row + q);
          if (a.out_col) __builtin_nontemporal_store((int32_t)(n0 + slot % SQ_C), a.out_col + q);
          const int f = s.first[slot];
          if (f >= 0) sq_close(a, s, slot, sigma, pos + 1, f, n0 + slot % SQ_C);
        }
      }
      __syncthreads();
    }
    if (a.records) {                                                       // four lanes per slot: one 16-byte piece each
      const int pieces = (a.row_words - win * SQ_WIN) >> 2;                // (of this window; row_words is a multiple of 4)
      const int piece = (int)threadIdx.x & 3;
#pragma unroll
      for (int i = 0; i < SQ_SLOTS * 4 / SQ_THREADS; ++i) {
        const int slot = i * (SQ_THREADS / 4) + ((int)threadIdx.x >> 2);
        const int64_t q = s.q[slot];
        const sq_u32x4 u = *reinterpret_cast<const sq_u32x4*>(&s.rec[slot * SQ_STRIDE + piece * 4]);
        if (q >= 0 && piece < pieces)
          __builtin_nontemporal_store(u, reinterpret_cast<sq_u32x4*>(a.records + (q * a.row_words + win * SQ_WIN + piece * 4)));
      }
    }
    if (win == 0) sq_pad(a, s, lane, wave);
    __syncthreads();
    if (!more) break;
    t0 = nt0;
    win = nwin;
  }
  // what is still open after row T - 1 closes here
  if (threadIdx.x == 0) s.pad_n = 0;
  __syncthreads();
  if (threadIdx.x < SQ_C && len > 0) {
    const int64_t sigma = shuffled ? sq_perm(seq, Q, h, mask, keys) : seq;
    s.q[threadIdx.x] = sigma * L + (len - 1);                              // (the last chunk's slots are dead: the column's own serves)
    s.pos[threadIdx.x] = len - 1;
    sq_close(a, s, (int)threadIdx.x, sigma, len, first, n0 + threadIdx.x);
  }
  __syncthreads();
  sq_pad(a, s, lane, wave);
}

extern "C" int phx_seq_batch(const phx_seq_batch_io* io, void* stream) {
  const char* fn = "phx_seq_batch";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_batch_shape(fn, *io, SQ_C)) return rc;
  if (io->max_seq_len < 1 || io->max_seq_len > PHX_SEQ_MAX_LEN)
    return fail(PHX_EINVAL, "phx_seq_batch: max_seq_len = %lld must lie in [1, %d]", (long long)io->max_seq_len, PHX_SEQ_MAX_LEN);
  if (const int rc = frag_batch_record(fn, *io, PHX_BATCH_MAX_PLANES)) return rc;
  if (io->capacity > (1LL << 62) / io->max_seq_len)
    return fail(PHX_EINVAL, "phx_seq_batch: capacity * max_seq_len = %lld * %lld must be <= 2^62", (long long)io->capacity, (long long)io->max_seq_len);
  if (const int rc = frag_batch_buffers(fn, *io, io->seq_start, "seq_start")) return rc;
  if ((io->out_col || io->seq_col) && io->N > 0x7fffffffLL)
    return fail(PHX_EINVAL, "phx_seq_batch: out_col and seq_col need N = %lld <= 2^31 - 1", (long long)io->N);
  if (const int rc = frag_batch_planes(fn, *io)) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->seq_start, io->records, io->out_row, io->out_col, io->moments, io->workspace, io->seq_lens,
                                                io->seq_row, io->seq_col),
                                  16, "seq_start, records, out_row, out_col, seq_lens, seq_row, seq_col, moments and workspace"))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  const bool has_std = io->std_plane >= 0;
  const float* x = has_std ? static_cast<const float*>(io->plane[io->std_plane].src) : nullptr;
  double* sums = static_cast<double*>(io->workspace);                      // [N][2] f64, then the kept rows [N] i64
  int64_t* rows = has_std ? reinterpret_cast<int64_t*>(sums + 2 * io->N) : nullptr;
  hipLaunchKernelGGL(phx_seq_count_kernel, dim3((unsigned)((io->N + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st, io->keep, io->col_class,
                     io->terminated, io->truncated, x, io->seq_start, sums, rows, (int)io->T, io->N, io->S, io->class_id, (int)io->max_seq_len);
  if (const int rc = call.launched("the count", "phx_seq_count_kernel")) return rc;
  hipLaunchKernelGGL(phx_seq_scan_kernel, dim3(1), dim3(SS_THREADS), 0, st, io->seq_start, io->N);
  if (const int rc = call.launched("the scan", "phx_seq_scan_kernel")) return rc;
  if (has_std) {
    hipLaunchKernelGGL(phx_seq_moments_kernel, dim3(1), dim3(SM_THREADS), 0, st, static_cast<const double*>(sums), static_cast<const int64_t*>(rows),
                       io->moments, io->N);
    if (const int rc = call.launched("the moments", "phx_seq_moments_kernel")) return rc;
  }
  if (io->capacity == 0 || (!io->records && !io->out_row && !io->out_col && !io->seq_lens && !io->seq_row && !io->seq_col))
    return PHX_OK;                                                         // (nothing to write)
  SqKeys keys;
  frag_round_keys(io->seed, io->epoch, keys.key);
  hipLaunchKernelGGL(phx_seq_scatter_kernel, dim3((unsigned)((io->N + SQ_C - 1) / SQ_C)), dim3(SQ_THREADS), 0, st, *io, keys);
  return call.launched("the scatter", "phx_seq_scatter_kernel");
}
