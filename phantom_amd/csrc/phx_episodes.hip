// phx_episodes.hip -- phx_episode_stats (include/phantom_amd_episodes.h): the returns and lengths of the episodes that close inside a
// rollout fragment, with a carry per output column for the episode the fragment cuts, per-column statistics and (a second launch) a
// fixed-order reduction of them into per-class ones.  Two small kernels on one stream inside the one call:
//
// phx_episode_scan_kernel: a forward scan over the T rows of an output column with a few words of state: the open episode's return
// and length and the column's statistics of this call.  The mapping and the discipline are phx_gae_masked_kernel's
// (phx_gae_masked.hip, which this file leaves alone):
//   * a lane owns ONE output column and a wave 64 consecutive ones, one wave per workgroup.  With G = 1 (GROUPED = false) every row
//     access of a wave is one coalesced 256-byte (f32) or 64-byte (u8) piece at any alignment of the inputs and for any N (lanes
//     past C leave at entry).  With G > 1 (GROUPED = true) the SAME lane walks its G input columns in ascending order -- the header
//     defines the return by that fold order, so one lane does the adds of an output column -- and a wave's access is 64 elements G
//     apart: G times the lines per load, each line read again by the next G - 1 loads (expected to hit in cache);
//   * the scan consumes ITEMS, the (row, member) pairs of the column in (t, g) order, EP_K at a time: the loads of EP_K items are
//     issued a chunk ahead into the second of two register buffers, then the chain of the current chunk runs, with its stores.  Loads
//     and stores share vmcnt on gfx950: the next chunk's loads are issued BEFORE this chunk's stores, and no load sits behind a
//     data-dependent branch -- items past the last are clamped to the last (loaded again, never used), a NULL input plane is a
//     template parameter (8 instantiations per mapping), a NULL output is a uniform branch around a store;
//   * EP_K = 8: an item is up to five loads and a row two stores.  When the wave waits for chunk c + 1's loads, what it has issued
//     after them is chunk c's stores and chunk c + 2's loads, at most 8 * (2 + 5) = 56 operations, which the six-bit vmcnt (63)
//     counts exactly;
//   * the row step is selects only: a row that closes nothing computes what a closing row computes and stores +0.0 and -1, so that
//     the two per-row planes are written everywhere.  Non-temporal stores for them: they are never read again here.  col_stats and
//     the carry are plain stores: the reduction reads col_stats next, the next call reads the carry.
//
// phx_episode_reduce_kernel (only with `summary`): one 256-thread workgroup per class k.  Lane i folds the columns j = i, i + 256, ..
// of the class (c = j * K + k) into its own value starting from the empty one, then a tree over LDS halves the lanes from h = 128
// down to 1 -- the header's order, for any M and without scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_episodes.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int EP_K = 8;            // items per chunk of the scan (tests/test_gpu_episode_stats.py walks T below, at and across it)
constexpr int EP_LANES = 64;       // output columns per workgroup of the scan: one wave
constexpr int EP_RED = 256;        // the reduction's workgroup: the header's 256 lane values
constexpr int EP_MAX_G = 256;

using EpStats = struct phx_episode_stats;

__device__ __forceinline__ EpStats ep_empty() {
  EpStats s;
  s.count = 0; s.len_sum = 0;
  s.ret_sum = 0.0; s.ret_sumsq = 0.0;
  s.ret_min = __builtin_inff(); s.ret_max = -__builtin_inff();
  s.len_min = 0x7fffffff; s.len_max = -1;
  return s;
}

template <bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
struct EpChunk {
  float r[EP_K];
  uint32_t tr[EP_K], te[HAS_TERM ? EP_K : 1], ac[HAS_ACT ? EP_K : 1], rv[HAS_RV ? EP_K : 1];
};

// the load stream of an output column: element offset `o` of item (t, g), walked an item at a time and held at the last item
struct EpStream {
  int64_t o;
  int t, g;
  __device__ __forceinline__ EpStream(const phx_episode_io& a, const int64_t c) : o(c * a.G), t(0), g(0) {}
  template <bool GROUPED>
  __device__ __forceinline__ void next(const phx_episode_io& a) {
    if (GROUPED) {
      const bool in_row = g + 1 < a.G;                   // (wave-uniform, as is every value here but o's base)
      const bool more = t + 1 < a.T;
      o += in_row ? 1 : (more ? a.N - (a.G - 1) : 0);
      t += !in_row && more ? 1 : 0;
      g = in_row ? g + 1 : (more ? 0 : g);
    } else {
      const bool more = t + 1 < a.T;
      o += more ? a.N : 0;
      t += more ? 1 : 0;
    }
  }
};

// the next EP_K items of the stream (items past the last: the last again)
template <bool GROUPED, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__device__ __forceinline__ void ep_load(EpChunk<HAS_TERM, HAS_ACT, HAS_RV>& c, const phx_episode_io& a, EpStream& p) {
#pragma unroll
  for (int k = 0; k < EP_K; ++k) {
    c.r[k] = a.reward[p.o];
    c.tr[k] = a.truncated[p.o];
    if (HAS_TERM) c.te[k] = a.terminated[p.o];
    if (HAS_ACT) c.ac[k] = a.acted[p.o];
    if (HAS_RV) c.rv[k] = a.reward_valid[p.o];
    p.next<GROUPED>(a);
  }
}

// what an output column carries from item to item (the header's definition, same names) and where its next row's outputs go
struct EpState {
  float ret;
  int32_t len;
  bool any_act = false, all_flag = true;
  int t = 0, g = 0;                                      // the item the chain consumes next
  int64_t out;                                           // t * C + c
  EpStats col;
};

// the definition for the chunk's items that exist
template <bool GROUPED, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__device__ __forceinline__ void ep_chain(const EpChunk<HAS_TERM, HAS_ACT, HAS_RV>& c, const phx_episode_io& a, const int64_t C, EpState& s) {
#pragma unroll
  for (int k = 0; k < EP_K; ++k) {
    if (s.t >= a.T) break;                               // (wave-uniform, and around stores only)
    const bool present = !HAS_RV || c.rv[k] == 1;
    const bool act = !HAS_ACT || c.ac[k] != 0;
    const bool opens = (present || act) && s.len < 0;
    s.ret = opens ? 0.0f : s.ret;
    s.len = opens ? 0 : s.len;
    s.ret = present ? s.ret + c.r[k] : s.ret;
    s.any_act = s.any_act || act;
    s.all_flag = s.all_flag && ((HAS_TERM && c.te[k] != 0) || c.tr[k] != 0);
    if (GROUPED && s.g + 1 < a.G) {                      // (wave-uniform: the row goes on)
      s.g += 1;
      continue;
    }
    s.len += s.any_act ? 1 : 0;
    const bool closes = s.all_flag && s.len >= 0;
    if (a.episode_return) __builtin_nontemporal_store(closes ? s.ret : 0.0f, a.episode_return + s.out);
    if (a.episode_len) __builtin_nontemporal_store(closes ? s.len : -1, a.episode_len + s.out);
    const double d = (double)s.ret;
    s.col.count += closes ? 1 : 0;
    s.col.len_sum += closes ? s.len : 0;
    s.col.ret_sum = closes ? s.col.ret_sum + d : s.col.ret_sum;
    s.col.ret_sumsq = closes ? s.col.ret_sumsq + d * d : s.col.ret_sumsq;
    s.col.ret_min = closes && s.ret < s.col.ret_min ? s.ret : s.col.ret_min;
    s.col.ret_max = closes && s.ret > s.col.ret_max ? s.ret : s.col.ret_max;
    s.col.len_min = closes && s.len < s.col.len_min ? s.len : s.col.len_min;
    s.col.len_max = closes && s.len > s.col.len_max ? s.len : s.col.len_max;
    s.ret = closes ? 0.0f : s.ret;
    s.len = closes ? -1 : s.len;
    s.any_act = false;
    s.all_flag = true;
    s.g = 0;
    s.t += 1;
    s.out += C;
  }
}

template <bool GROUPED, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__global__ __launch_bounds__(EP_LANES) void phx_episode_scan_kernel(const phx_episode_io a, const int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * EP_LANES + threadIdx.x;
  if (c >= C) return;
  EpChunk<HAS_TERM, HAS_ACT, HAS_RV> c0, c1;
  EpStream p(a, c);
  EpState s;
  s.ret = 0.0f;
  s.len = -1;
  if (a.carry_return) {                                  // (uniform; the one load ahead of the stream)
    s.ret = a.carry_return[c];
    s.len = a.carry_len[c];
  }
  s.out = c;
  s.col = ep_empty();
  ep_load<GROUPED>(c0, a, p);
  for (;;) {
    ep_load<GROUPED>(c1, a, p);
    ep_chain<GROUPED>(c0, a, C, s);
    if (s.t >= a.T) break;
    ep_load<GROUPED>(c0, a, p);
    ep_chain<GROUPED>(c1, a, C, s);
    if (s.t >= a.T) break;
  }
  if (a.carry_return) {
    a.carry_return[c] = s.ret;
    a.carry_len[c] = s.len;
  }
  a.col_stats[c] = s.col;
}

__device__ __forceinline__ void ep_combine(EpStats& x, const EpStats& y) {
  x.count += y.count;
  x.len_sum += y.len_sum;
  x.ret_sum = x.ret_sum + y.ret_sum;
  x.ret_sumsq = x.ret_sumsq + y.ret_sumsq;
  x.ret_min = y.ret_min < x.ret_min ? y.ret_min : x.ret_min;
  x.ret_max = y.ret_max > x.ret_max ? y.ret_max : x.ret_max;
  x.len_min = y.len_min < x.len_min ? y.len_min : x.len_min;
  x.len_max = y.len_max > x.len_max ? y.len_max : x.len_max;
}

__global__ __launch_bounds__(EP_RED) void phx_episode_reduce_kernel(const phx_episode_io a, const int64_t M) {
  __shared__ EpStats lane[EP_RED];
  const int i = (int)threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x;
  EpStats x = ep_empty();
  for (int64_t j = i; j < M; j += EP_RED) ep_combine(x, a.col_stats[j * a.K + k]);
  lane[i] = x;
  __syncthreads();
  for (int h = EP_RED / 2; h >= 1; h >>= 1) {
    if (i < h) {
      ep_combine(x, lane[i + h]);
      lane[i] = x;
    }
    __syncthreads();
  }
  if (i == 0) a.summary[k] = x;
}

// instantiation W: bit 3 grouped (G > 1), bit 2 terminated, bit 1 acted, bit 0 reward_valid given
template <int W>
static void ep_launch(const int which, const phx_episode_io& io, const int64_t C, hipStream_t st) {
  if (which == W) {
    const unsigned grid = (unsigned)((C + EP_LANES - 1) / EP_LANES);
    hipLaunchKernelGGL((phx_episode_scan_kernel<(W & 8) != 0, (W & 4) != 0, (W & 2) != 0, (W & 1) != 0>), dim3(grid), dim3(EP_LANES), 0, st, io, C);
  } else if constexpr (W > 0) {
    ep_launch<W - 1>(which, io, C, st);
  }
}

extern "C" int phx_episode_stats(const phx_episode_io* io, void* stream) {
  const char* fn = "phx_episode_stats";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_reserved0(fn, io->reserved0)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (io->G < 1 || io->G > EP_MAX_G) return fail(PHX_EINVAL, "phx_episode_stats: G = %d must lie in [1, %d]", io->G, EP_MAX_G);
  if (io->N % io->G != 0) return fail(PHX_EINVAL, "phx_episode_stats: N = %lld must be a multiple of G = %d", (long long)io->N, io->G);
  const int64_t C = io->N / io->G;
  if (io->K < 1 || C % io->K != 0)
    return fail(PHX_EINVAL, "phx_episode_stats: K = %d must be >= 1 and divide the %lld output columns", io->K, (long long)C);
  if (C > (int64_t)EP_LANES * 0x7fffffff) return frag_beyond_grid(fn, "%lld output columns are", (long long)C);
  if (const int rc = frag_required(fn, io->reward && io->truncated && io->col_stats, "reward, truncated and col_stats")) return rc;
  if ((io->carry_return == nullptr) != (io->carry_len == nullptr))
    return fail(PHX_EINVAL, "phx_episode_stats: carry_return and carry_len come together");
  if (const int rc = frag_aligned(fn, frag_bits(io->reward, io->carry_return, io->carry_len), 4, "reward, carry_return and carry_len")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->episode_return, io->episode_len, io->col_stats, io->summary), 16,
                                  "episode_return, episode_len, col_stats and summary"))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  const int which = (io->G > 1 ? 8 : 0) | (io->terminated ? 4 : 0) | (io->acted ? 2 : 0) | (io->reward_valid ? 1 : 0);
  ep_launch<15>(which, *io, C, st);
  if (const int rc = call.launched("the scan", "phx_episode_scan_kernel")) return rc;
  if (io->summary) {
    hipLaunchKernelGGL(phx_episode_reduce_kernel, dim3((unsigned)io->K), dim3(EP_RED), 0, st, *io, C / io->K);
    if (const int rc = call.launched("the reduction", "phx_episode_reduce_kernel")) return rc;
  }
  return PHX_OK;
}
