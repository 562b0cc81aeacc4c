// phx_traj_compact.hip -- phx_traj_compact (include/phantom_amd_compact.h): the kept elements of time-major planes, dense and in
// (column, row) order -- a stream compaction fused with the time-major to agent-major transpose.  Three launches on one stream
// (DESIGN 3.4i):
//
// phx_compact_count_kernel: a lane owns ONE column and a wave 64 consecutive ones (phx_traj_next_kernel's coalesced 64-byte row
//   pieces, lanes past N leave at entry); it walks the T rows of `keep` CC_K at a time, loads only (rows past the last are clamped
//   to it: loaded again, never counted), and leaves count[n] in start[n]: `start` is the call's only scratch.
// phx_compact_scan_kernel: the exclusive i64 prefix over start[0 .. N] in place, by ONE workgroup that carries its sum across blocks
//   of CP_SB entries; the next block's loads are issued before this block's stores (they never touch the same entries).
// phx_compact_scatter_kernel: a workgroup owns a tile of CP_C consecutive columns and walks T in chunks of CP_R rows.
//   * every piece of work is an ITEM: the chunk's keep bytes, then for every plane the column groups of the tile (a group is as many
//     columns as put at most 64 words into a row: 64 / w of a w-word plane, all CP_C of a byte plane).  An item is loaded ROW-WISE --
//     a wave-instruction reads one row's contiguous piece, coalesced whatever N is -- into 16 registers per lane, then written to LDS
//     (row stride padded by one word against bank conflicts);
//   * the NEXT item's loads are issued before this item's stores (loads and stores share vmcnt on gfx950, 3.2b), unconditionally: rows
//     past T are clamped to T - 1, words past the tile's last column to its last word, and after the last item the same item is
//     loaded once more -- no global load sits behind a branch of the store phase;
//   * the keep item: a wave owns one column at a time, its lanes on the chunk's rows: one 64-bit ballot, the lane's rank by mbcnt,
//     the column's running base = start[n] (read once) + the popcounts of the earlier chunks.  Mask, base and the list of kept rows
//     stay in LDS for every plane of the chunk: computed once per tile and chunk.  out_row / out_col are written here (template
//     parameters: four instantiations of this kernel, which with the count and the scan makes six in this file);
//   * a plane item: a wave owns one column at a time and its lanes the WORDS of the column's run -- lane = (kept element, word): a
//     store instruction covers consecutive addresses also for w > 1.  Byte planes take the same path with bytes for words;
//   * non-temporal stores: nothing on the device reads dst again.  The capacity clip is a predicate on the store only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_compact.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int CP_R = 64;             // rows per chunk of the scatter: a wave's lanes (tests/test_gpu_compact.py walks T around it)
constexpr int CP_C = 64;             // columns per tile of the scatter
constexpr int CP_SB = 4096;          // entries per block of the scan: 4 consecutive ones per thread (16 per thread took 1.7-1.9x: DESIGN 3.4i)
constexpr int CP_THREADS = 256;      // the scatter's workgroup: four waves
constexpr int CP_WAVES = CP_THREADS / 64;
constexpr int CP_LD = CP_R / CP_WAVES;          // rows a wave loads per item: registers per lane
constexpr int CP_WSTRIDE = 65;       // words per tile row in LDS (64 + 1)
constexpr int CP_BSTRIDE = 68;       // bytes per tile row in LDS (64 + 4)
constexpr int CC_THREADS = 256;      // the count's workgroup
constexpr int CC_K = 8;              // rows per chunk of the count
constexpr int CS_THREADS = 1024;     // the scan's workgroup
constexpr int CS_ITEMS = CP_SB / CS_THREADS;

__global__ __launch_bounds__(CC_THREADS) void phx_compact_count_kernel(const uint8_t* __restrict__ keep, int64_t* __restrict__ start,
                                                                       const int T, const int64_t N) {
  const int64_t n = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (n >= N) return;
  const uint8_t* p = keep + n;
  uint32_t cnt = 0;
  for (int t0 = 0; t0 < T; t0 += CC_K) {
    uint32_t v[CC_K];
#pragma unroll
    for (int k = 0; k < CC_K; ++k) {
      const int t = t0 + k < T ? t0 + k : T - 1;
      v[k] = p[(int64_t)t * N];
    }
#pragma unroll
    for (int k = 0; k < CC_K; ++k) cnt += (t0 + k < T && v[k] != 0) ? 1u : 0u;
  }
  start[n] = (int64_t)cnt;
}

// entries [i0, i0 + CP_SB) of the counts, CS_ITEMS consecutive ones per thread; entry N and beyond: 0 (start[N] holds no count)
__device__ __forceinline__ void cs_load(int64_t (&v)[CS_ITEMS], const int64_t* start, const int64_t i0, const int64_t N) {
#pragma unroll
  for (int e = 0; e < CS_ITEMS; ++e) {
    const int64_t i = i0 + (int64_t)threadIdx.x * CS_ITEMS + e;
    v[e] = i < N ? start[i] : 0;
  }
}

__global__ __launch_bounds__(CS_THREADS) void phx_compact_scan_kernel(int64_t* start, const int64_t N) {
  __shared__ int64_t wsum[CS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  int64_t v[CS_ITEMS], nx[CS_ITEMS];
  cs_load(v, start, 0, N);
  for (int64_t i0 = 0; i0 <= N; i0 += CP_SB) {
    cs_load(nx, start, i0 + CP_SB, N);
    int64_t s = 0;
#pragma unroll
    for (int e = 0; e < CS_ITEMS; ++e) s += v[e];
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
    for (int j = 0; j < CS_THREADS / 64; ++j) {
      const int64_t x = wsum[j];
      before += j < wave ? x : 0;
      total += x;
    }
    int64_t ex = carry + before + inc - s;
#pragma unroll
    for (int e = 0; e < CS_ITEMS; ++e) {
      const int64_t i = i0 + (int64_t)threadIdx.x * CS_ITEMS + e;
      if (i <= N) start[i] = ex;
      ex += v[e];
    }
    carry += total;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < CS_ITEMS; ++e) v[e] = nx[e];
  }
}

// one piece of the scatter's work: chunk rows [t0, t0 + CP_R), plane k (-1: the keep bytes), column group g of the tile
struct CpItem {
  int t0, k, g;
};

// a plane's words per element (a byte plane: 1) and columns per group
__device__ __forceinline__ int cp_words(const phx_traj_compact_io& a, const int k) {
  const int eb = a.plane[k].elem_bytes;
  return eb == 1 ? 1 : eb >> 2;
}

struct CpTile {
  uint32_t words[CP_R * CP_WSTRIDE];            // a plane item's rows (a byte plane's: CP_BSTRIDE bytes per row, in the same memory)
  uint8_t keep[CP_R * CP_BSTRIDE];              // the chunk's keep bytes
  uint8_t rows[CP_C * CP_R];                    // [column][rank]: the chunk row of the column's rank-th kept element
  uint64_t mask[CP_C];                          // the chunk's ballot per column
  int64_t base[CP_C];                           // the position of the column's first kept element of the chunk
};

// the item's rows, row-wise: row wave * CP_LD + i of the chunk in v[i], this lane's word (byte) of the row's piece
__device__ __forceinline__ void cp_load(uint32_t (&v)[CP_LD], const phx_traj_compact_io& a, const CpItem it, const int64_t n0, const int ncol,
                                        const int lane, const int wave) {
  const int r0 = it.t0 + wave * CP_LD;
  if (it.k < 0 || a.plane[it.k < 0 ? 0 : it.k].elem_bytes == 1) {         // (workgroup-uniform; the load phase)
    const uint8_t* src = it.k < 0 ? a.keep : static_cast<const uint8_t*>(a.plane[it.k].src);
    const int64_t o = n0 + (lane < ncol ? lane : ncol - 1);
#pragma unroll
    for (int i = 0; i < CP_LD; ++i) {
      const int t = r0 + i < a.T ? r0 + i : a.T - 1;
      v[i] = src[(int64_t)t * a.N + o];
    }
  } else {
    const int w = cp_words(a, it.k);
    const int G = 64 / w, g0 = it.g * G;
    const int width = (ncol - g0 < G ? ncol - g0 : G) * w;
    const uint32_t* src = static_cast<const uint32_t*>(a.plane[it.k].src);
    const int64_t o = (n0 + g0) * w + (lane < width ? lane : width - 1);
    const int64_t pitch = a.N * w;
#pragma unroll
    for (int i = 0; i < CP_LD; ++i) {
      const int t = r0 + i < a.T ? r0 + i : a.T - 1;
      v[i] = src[(int64_t)t * pitch + o];
    }
  }
}

__device__ __forceinline__ void cp_to_lds(const uint32_t (&v)[CP_LD], CpTile& s, const bool is_keep, const bool bytes, const int lane, const int wave) {
  uint8_t* tb = is_keep ? s.keep : reinterpret_cast<uint8_t*>(s.words);
#pragma unroll
  for (int i = 0; i < CP_LD; ++i) {
    const int r = wave * CP_LD + i;
    if (bytes) tb[r * CP_BSTRIDE + lane] = (uint8_t)v[i];
    else s.words[r * CP_WSTRIDE + lane] = v[i];
  }
}

// the item after `it`; false: there is none
__device__ __forceinline__ bool cp_next(CpItem& it, const phx_traj_compact_io& a, const int ncol) {
  if (it.k >= 0 && a.plane[it.k].elem_bytes != 1) {
    const int G = 64 / cp_words(a, it.k);
    if ((it.g + 1) * G < ncol) {
      ++it.g;
      return true;
    }
  }
  ++it.k;
  it.g = 0;
  if (it.k >= a.n_planes) {
    it.k = -1;
    it.t0 += CP_R;
  }
  return it.t0 < a.T;
}

// the keep item: ballots, ranks, bases and kept-row lists of the chunk; out_row / out_col
template <bool HAS_ROW, bool HAS_COL>
__device__ __forceinline__ void cp_rank(CpTile& s, const phx_traj_compact_io& a, const int t0, const int64_t n0, const int ncol, const int lane,
                                        const int wave) {
  for (int c = wave; c < CP_C; c += CP_WAVES) {
    const bool kp = c < ncol && t0 + lane < a.T && s.keep[lane * CP_BSTRIDE + c] != 0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(kp);
    const int64_t b = s.base[c] + __popcll(s.mask[c]);                     // (the previous chunk's; zero before the first)
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) {
      s.base[c] = b;
      s.mask[c] = m;
    }
    if (kp) s.rows[c * CP_R + rank] = (uint8_t)lane;
    const int64_t p = b + rank;
    if ((HAS_ROW || HAS_COL) && kp && p < a.capacity) {
      if (HAS_ROW) __builtin_nontemporal_store((int32_t)(t0 + lane), a.out_row + p);
      if (HAS_COL) __builtin_nontemporal_store((int32_t)(n0 + c), a.out_col + p);
    }
  }
}

// a plane item: the kept elements of the group's columns, each column's as one contiguous run of words (bytes)
template <typename E, int STRIDE>
__device__ __forceinline__ void cp_store(const CpTile& s, const phx_traj_compact_io& a, const CpItem it, const int w, const int ncol, const int lane,
                                         const int wave) {
  const E* tile = reinterpret_cast<const E*>(s.words);
  E* dst = static_cast<E*>(a.plane[it.k].dst);
  const int G = 64 / w, g0 = it.g * G;
  const int g1 = ncol - g0 < G ? ncol : g0 + G;                            // the group's columns: [g0, g1)
  const int ksub = lane / w, d = lane - ksub * w;                          // this lane's element of a store instruction and its word
  const bool active = ksub < G;                                            // (G elements per instruction: G * w <= 64 lanes)
  for (int c = g0 + ((wave - g0) & (CP_WAVES - 1)); c < g1; c += CP_WAVES) {          // (column c is wave c % CP_WAVES's, as in cp_rank)
    const uint64_t m = s.mask[c];
    const int kc = __builtin_amdgcn_readfirstlane(__popcll(m));
    const int64_t b = s.base[c];
    for (int k0 = 0; k0 < kc; k0 += G) {
      const int k = k0 + ksub;
      const bool ok = active && k < kc;
      const int row = s.rows[c * CP_R + (ok ? k : 0)];
      const E v = tile[row * STRIDE + (c - g0) * w + d];
      const int64_t p = b + k;
      if (ok && p < a.capacity) __builtin_nontemporal_store(v, dst + (p * w + d));
    }
  }
}

template <bool HAS_ROW, bool HAS_COL>
__global__ __launch_bounds__(CP_THREADS) void phx_compact_scatter_kernel(const phx_traj_compact_io a) {
  __shared__ CpTile s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * CP_C;
  const int ncol = (int)(a.N - n0 < CP_C ? a.N - n0 : CP_C);
  if (threadIdx.x < CP_C) {                                                // (read by the columns' waves after the loop's first barrier)
    s.base[threadIdx.x] = (int)threadIdx.x < ncol ? a.start[n0 + threadIdx.x] : 0;
    s.mask[threadIdx.x] = 0;
  }
  CpItem it{0, -1, 0};
  uint32_t v[CP_LD];
  cp_load(v, a, it, n0, ncol, lane, wave);
  for (;;) {
    const bool is_keep = it.k < 0;
    const int eb = is_keep ? 1 : a.plane[it.k].elem_bytes;
    cp_to_lds(v, s, is_keep, eb == 1, lane, wave);
    __syncthreads();
    CpItem nx = it;
    const bool more = cp_next(nx, a, ncol);
    cp_load(v, a, more ? nx : it, n0, ncol, lane, wave);                   // (after the last item: the same one again, never used)
    if (is_keep) cp_rank<HAS_ROW, HAS_COL>(s, a, it.t0, n0, ncol, lane, wave);
    else if (eb == 1) cp_store<uint8_t, CP_BSTRIDE>(s, a, it, 1, ncol, lane, wave);
    else cp_store<uint32_t, CP_WSTRIDE>(s, a, it, eb >> 2, ncol, lane, wave);
    __syncthreads();
    if (!more) break;
    it = nx;
  }
}

template <bool HAS_ROW, bool HAS_COL>
static void cp_launch(const phx_traj_compact_io& io, hipStream_t st) {
  const unsigned grid = (unsigned)((io.N + CP_C - 1) / CP_C);
  hipLaunchKernelGGL((phx_compact_scatter_kernel<HAS_ROW, HAS_COL>), dim3(grid), dim3(CP_THREADS), 0, st, io);
}

extern "C" int phx_traj_compact(const phx_traj_compact_io* io, void* stream) {
  const char* fn = "phx_traj_compact";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, CP_C)) return rc;
  if (const int rc = frag_n_planes(fn, io->n_planes, PHX_COMPACT_MAX_PLANES)) return rc;
  if (const int rc = frag_at_least(fn, "capacity", io->capacity, 0)) return rc;
  if (const int rc = frag_required(fn, io->keep && io->start, "keep and start")) return rc;
  if (io->out_col && io->N > 0x7fffffffLL) return fail(PHX_EINVAL, "phx_traj_compact: out_col needs N = %lld <= 2^31 - 1", (long long)io->N);
  uintptr_t align16 = frag_bits(io->start, io->out_row, io->out_col);
  for (int k = 0; k < io->n_planes; ++k) {
    const phx_compact_plane& p = io->plane[k];
    if (!p.src || !p.dst) return fail(PHX_EINVAL, "phx_traj_compact: plane %d needs src and dst", k);
    if (const int rc = frag_plane_elem(fn, k, p.elem_bytes)) return rc;
    if (p.reserved != 0) return fail(PHX_EINVAL, "phx_traj_compact: plane %d: reserved must be 0", k);
    if (const int rc = frag_plane_src(fn, k, p.src, p.elem_bytes)) return rc;
    align16 |= (uintptr_t)p.dst;
  }
  if (const int rc = frag_aligned(fn, align16, 16, "start, out_row, out_col and every dst")) return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  hipLaunchKernelGGL(phx_compact_count_kernel, dim3((unsigned)((io->N + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, io->keep, io->start,
                     io->T, io->N);
  if (const int rc = call.launched("the count", "phx_compact_count_kernel")) return rc;
  hipLaunchKernelGGL(phx_compact_scan_kernel, dim3(1), dim3(CS_THREADS), 0, st, io->start, io->N);
  if (const int rc = call.launched("the scan", "phx_compact_scan_kernel")) return rc;
  if (io->capacity == 0 || (io->n_planes == 0 && !io->out_row && !io->out_col)) return PHX_OK;      // (nothing to write)
  if (io->out_row) {
    if (io->out_col) cp_launch<true, true>(*io, st); else cp_launch<true, false>(*io, st);
  } else {
    if (io->out_col) cp_launch<false, true>(*io, st); else cp_launch<false, false>(*io, st);
  }
  return call.launched("the scatter", "phx_compact_scatter_kernel");
}
