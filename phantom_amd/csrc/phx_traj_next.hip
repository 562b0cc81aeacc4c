// phx_traj_next.hip -- phx_traj_next (include/phantom_amd_traj.h): for every row where an agent of an FSM / Stackelberg fragment acted,
// the row whose observation it holds when its transition ends, the transition's done flags and (a second launch) that observation.
//
// phx_traj_next_kernel is the same reverse scan over the T rows of a column as phx_gae_masked_kernel (phx_gae_masked.hip, which this
// file leaves alone), over the same segments, with three words of state per column and no arithmetic at all.  The mapping and the
// discipline are phx_vtrace_kernel's (what is this kernel's own: DESIGN 3.4h):
//   * a lane owns ONE column and a wave 64 consecutive ones, one wave per workgroup: every row access of a wave is one coalesced
//     64-byte (u8) or 256-byte (i32) piece at any alignment of the inputs and for any N (lanes past N leave at entry);
//   * the loads of TN_K rows are issued a chunk ahead into the second of two register buffers, then the current chunk's row steps run,
//     then its stores.  Loads and stores share vmcnt on gfx950: the next chunk's loads are issued BEFORE this chunk's stores, and no
//     load sits behind a branch -- rows past the fragment's first are clamped to row 0 (loaded again, never used), a NULL input plane
//     is a template parameter (terminated, acted, new_obs_valid: eight instantiations);
//   * TN_K = 8, not 15.  A row is at most four byte loads and three stores.  When the wave waits for chunk c + 1's loads, what it has
//     issued AFTER them is chunk c's stores and chunk c + 2's loads: 8 * (3 + 4) = 56 operations, which the six-bit vmcnt (63) counts
//     exactly, so every wait ends inside chunk c + 1's own loads.  15 rows fit one chunk's loads into the counter (60) but put 105
//     operations behind them: the wait saturates and also waits for most of the stores that were issued to be hidden.  (Measured, the
//     two are level within 3 %; 8 rows take 88 registers where 15 take 110);
//   * addresses are running pointers, one per plane, stepped in place by a wave-uniform stride (TnStream): the load phase holds no wait;
//   * the flag bytes are held as they arrive, one register each: packing them is an operation on a loaded value, a wait in the load phase;
//   * the row step is selects only: a hole row computes what a trajectory row computes and stores (-1, 0, 0), so that the output planes
//     are written everywhere.  Non-temporal stores: the flag planes are never read again here, and the gather that may follow finds
//     next_row in L2 all the same.
//
// phx_traj_gather_kernel is the gather of next_obs, fully parallel over the T * N * D words: a data-dependent load (new_obs at
// next_row) has no place between the scan's stores (3.2b), so it is a launch of its own on the same stream inside the same call.  A
// thread owns one word of a row's N * D and TG_ROWS consecutive rows: it loads acted and next_row of its rows, then BOTH source words
// of each row unconditionally (the row clamped to 0 for -1) and selects -- words are moved as 32-bit integers, never computed with.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_traj.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int TN_K = 8;            // rows per chunk (tests/test_gpu_traj_next.py walks T below, at and across it)
constexpr int TN_LANES = 64;       // columns per workgroup: one wave
constexpr int TG_THREADS = 256;    // the gather's workgroup: 256 consecutive words of a row
constexpr int TG_ROWS = 4;         // rows per gather thread (the index arithmetic is paid once for them, their loads overlap)

template <bool HAS_TERM, bool HAS_ACT, bool HAS_NV>
struct TnChunk {
  uint32_t tr[TN_K], te[HAS_TERM ? TN_K : 1], ac[HAS_ACT ? TN_K : 1], nv[HAS_NV ? TN_K : 1];
};

// the load stream of a column: one pointer per input plane at row `t` of the column, walked down a row at a time and held at row 0
// (updated in place: no address is formed in a temporary register -- phx_vtrace.hip's VtStream)
template <bool HAS_TERM, bool HAS_ACT, bool HAS_NV>
struct TnStream {
  const uint8_t *tr, *te, *ac, *nv;
  int t;
  __device__ __forceinline__ TnStream(const phx_traj_next_io& a, const int64_t n) : t(a.T - 1) {
    const int64_t o = (int64_t)t * a.N + n;
    tr = a.truncated + o;
    te = HAS_TERM ? a.terminated + o : nullptr;
    ac = HAS_ACT ? a.acted + o : nullptr;
    nv = HAS_NV ? a.new_obs_valid + o : nullptr;
  }
  __device__ __forceinline__ void down(const phx_traj_next_io& a) {
    const int64_t step = t > 0 ? -a.N : 0;               // (wave-uniform)
    t = t > 0 ? t - 1 : 0;
    tr += step;
    if (HAS_TERM) te += step;
    if (HAS_ACT) ac += step;
    if (HAS_NV) nv += step;
  }
};

// the next TN_K rows of the stream (rows below 0: row 0 again)
template <bool HAS_TERM, bool HAS_ACT, bool HAS_NV>
__device__ __forceinline__ void tn_load(TnChunk<HAS_TERM, HAS_ACT, HAS_NV>& c, const phx_traj_next_io& a, TnStream<HAS_TERM, HAS_ACT, HAS_NV>& p) {
#pragma unroll
  for (int k = 0; k < TN_K; ++k) {
    c.tr[k] = *p.tr;
    if (HAS_TERM) c.te[k] = *p.te;
    if (HAS_ACT) c.ac[k] = *p.ac;
    if (HAS_NV) c.nv[k] = *p.nv;
    p.down(a);
  }
}

// what a column carries from row t + 1 to row t (the header's scan, same names), and its elements of the output planes at row t
struct TnState {
  int32_t nr = -1;
  bool term = false, trunc = false;
  int32_t* row_out;
  uint8_t *term_out, *trunc_out;
};

// the header's scan for the chunk's rows that exist
template <bool HAS_TERM, bool HAS_ACT, bool HAS_NV>
__device__ __forceinline__ void tn_chain(const TnChunk<HAS_TERM, HAS_ACT, HAS_NV>& c, const phx_traj_next_io& a, const int t_hi, TnState& s) {
#pragma unroll
  for (int k = 0; k < TN_K; ++k) {
    const int t = t_hi - k;
    if (t < 0) break;                                    // (wave-uniform, and around stores only)
    const bool te = HAS_TERM && c.te[k] != 0;
    const bool tr = c.tr[k] != 0;
    const bool crow = te || tr || t == a.T - 1;
    const int32_t here = (!HAS_NV || c.nv[k] != 0) ? t : -1;
    s.nr = crow ? here : (s.nr < 0 ? here : s.nr);
    s.term = crow ? te : s.term;
    s.trunc = crow ? (!te && tr) : s.trunc;
    const bool act = !HAS_ACT || c.ac[k] != 0;
    __builtin_nontemporal_store(act ? s.nr : -1, s.row_out);
    __builtin_nontemporal_store((uint8_t)(act && s.term ? 1 : 0), s.term_out);
    __builtin_nontemporal_store((uint8_t)(act && s.trunc ? 1 : 0), s.trunc_out);
    s.nr = act ? -1 : s.nr;
    s.term = s.term && !act;
    s.trunc = s.trunc && !act;
    s.row_out += -a.N;
    s.term_out += -a.N;
    s.trunc_out += -a.N;
  }
}

template <bool HAS_TERM, bool HAS_ACT, bool HAS_NV>
__global__ __launch_bounds__(TN_LANES) void phx_traj_next_kernel(const phx_traj_next_io a) {
  const int64_t n = (int64_t)blockIdx.x * TN_LANES + threadIdx.x;
  if (n >= a.N) return;
  TnChunk<HAS_TERM, HAS_ACT, HAS_NV> c0, c1;
  TnStream<HAS_TERM, HAS_ACT, HAS_NV> p(a, n);
  TnState s;
  int t_hi = a.T - 1;
  const int64_t o = (int64_t)t_hi * a.N + n;
  s.row_out = a.next_row + o;
  s.term_out = a.next_terminated + o;
  s.trunc_out = a.next_truncated + o;
  tn_load(c0, a, p);
  for (;;) {
    tn_load(c1, a, p);
    tn_chain(c0, a, t_hi, s);
    t_hi -= TN_K;
    if (t_hi < 0) break;
    tn_load(c0, a, p);
    tn_chain(c1, a, t_hi, s);
    t_hi -= TN_K;
    if (t_hi < 0) break;
  }
}

// next_obs: word w of row t is word d = w % D of column n = w / D.  IDX: 32-bit where N * D fits (the division is then a short one)
template <typename IDX, bool HAS_ACT>
__global__ __launch_bounds__(TG_THREADS) void phx_traj_gather_kernel(const phx_traj_next_io a, const IDX row_words) {
  const IDX w = (IDX)blockIdx.x * TG_THREADS + threadIdx.x;
  if (w >= row_words) return;
  const IDX n = w / (IDX)a.D;
  const uint32_t* obs = reinterpret_cast<const uint32_t*>(a.obs);
  const uint32_t* nob = reinterpret_cast<const uint32_t*>(a.new_obs);
  uint32_t* out = reinterpret_cast<uint32_t*>(a.next_obs);
  const int64_t rw = (int64_t)row_words;
  // (groups of TG_ROWS rows, one per workgroup row of the grid; the grid has at most 65535 of them: a longer fragment goes round)
  for (int64_t t0 = (int64_t)blockIdx.y * TG_ROWS; t0 < a.T; t0 += (int64_t)gridDim.y * TG_ROWS) {
    int32_t nr[TG_ROWS];
    uint32_t ac[TG_ROWS], own[TG_ROWS], got[TG_ROWS];
#pragma unroll
    for (int r = 0; r < TG_ROWS; ++r) {                  // (rows past the fragment's last: row T - 1 again, never stored)
      const int64_t t = t0 + r < a.T ? t0 + r : a.T - 1;
      const int64_t e = t * a.N + (int64_t)n;
      nr[r] = a.next_row[e];
      ac[r] = HAS_ACT ? a.acted[e] : 1;
    }
#pragma unroll
    for (int r = 0; r < TG_ROWS; ++r) {
      const int64_t t = t0 + r < a.T ? t0 + r : a.T - 1;
      const int64_t src = nr[r] < 0 ? 0 : nr[r];         // (-1: row 0 is loaded and not selected; the scan wrote next_row < T)
      own[r] = obs[t * rw + (int64_t)w];
      got[r] = nob[src * rw + (int64_t)w];
    }
#pragma unroll
    for (int r = 0; r < TG_ROWS; ++r) {
      const int64_t t = t0 + r;
      if (t >= a.T) break;                               // (uniform, and around a store only)
      const uint32_t v = ac[r] != 0 ? (nr[r] >= 0 ? got[r] : own[r]) : 0u;
      __builtin_nontemporal_store(v, out + (t * rw + (int64_t)w));
    }
  }
}

// instantiation W: bit 2 terminated, bit 1 acted, bit 0 new_obs_valid given
template <int W>
static void tn_launch(const int which, const phx_traj_next_io& io, hipStream_t st) {
  if (which == W) {
    const unsigned grid = (unsigned)((io.N + TN_LANES - 1) / TN_LANES);
    hipLaunchKernelGGL((phx_traj_next_kernel<(W & 4) != 0, (W & 2) != 0, (W & 1) != 0>), dim3(grid), dim3(TN_LANES), 0, st, io);
  } else if constexpr (W > 0) {
    tn_launch<W - 1>(which, io, st);
  }
}

template <typename IDX>
static void tg_launch(const phx_traj_next_io& io, hipStream_t st) {
  const int64_t row_words = io.N * io.D;
  const dim3 grid((unsigned)((row_words + TG_THREADS - 1) / TG_THREADS), (unsigned)min((io.T + TG_ROWS - 1) / TG_ROWS, 65535));
  if (io.acted)
    hipLaunchKernelGGL((phx_traj_gather_kernel<IDX, true>), grid, dim3(TG_THREADS), 0, st, io, (IDX)row_words);
  else
    hipLaunchKernelGGL((phx_traj_gather_kernel<IDX, false>), grid, dim3(TG_THREADS), 0, st, io, (IDX)row_words);
}

extern "C" int phx_traj_next(const phx_traj_next_io* io, void* stream) {
  const char* fn = "phx_traj_next";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, TN_LANES)) return rc;
  if (const int rc = frag_required(fn, io->truncated && io->next_row && io->next_terminated && io->next_truncated,
                                   "truncated, next_row, next_terminated and next_truncated"))
    return rc;
  if (io->next_obs) {
    if (!io->obs || !io->new_obs) return fail(PHX_EINVAL, "phx_traj_next: next_obs needs both obs and new_obs");
    if (io->D < 1 || io->D > 64) return fail(PHX_EINVAL, "phx_traj_next: D = %d must lie in [1, 64] when next_obs is given", io->D);
    if (io->N * io->D > (int64_t)TG_THREADS * 0x7fffffff) return frag_beyond_grid(fn, "N = %lld with D = %d is", (long long)io->N, io->D);
    if (const int rc = frag_aligned(fn, frag_bits(io->obs, io->new_obs), 4, "obs and new_obs")) return rc;
  }
  if (const int rc = frag_aligned(fn, frag_bits(io->next_row, io->next_terminated, io->next_truncated, io->next_obs), 16,
                                  "next_row, next_terminated, next_truncated and next_obs"))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  const int which = (io->terminated ? 4 : 0) | (io->acted ? 2 : 0) | (io->new_obs_valid ? 1 : 0);
  tn_launch<7>(which, *io, st);
  if (const int rc = call.launched(nullptr, "phx_traj_next_kernel")) return rc;
  if (io->next_obs) {
    if (io->N * io->D <= 0xffffff00LL) tg_launch<uint32_t>(*io, st); else tg_launch<uint64_t>(*io, st);
    if (const int rc = call.launched("the gather", "phx_traj_gather_kernel")) return rc;
  }
  return PHX_OK;
}
