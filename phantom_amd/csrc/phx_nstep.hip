// phx_nstep.hip -- phx_nstep (include/phantom_amd_nstep.h): for every row where an agent acted, the discounted sum of the rewards of its
// next n transitions, the last transition folded, its done flags and next row, the discount to bootstrap with and (a third launch) the
// observation to bootstrap from.  Three small kernels on one stream inside the one call:
//
// phx_nstep_succ_kernel (only with `acted`): succ_row[t] = the column's next trajectory row after t.  A reverse scan over the T rows of
// a column with ONE word of state and no arithmetic; the mapping and the discipline are phx_traj_next_kernel's (phx_traj_next.hip, which
// this file leaves alone):
//   * a lane owns ONE column and a wave 64 consecutive ones, one wave per workgroup: every row access of a wave is one coalesced 64-byte
//     (u8) or 256-byte (i32) piece at any alignment of `acted` and for any N (lanes past N leave at entry);
//   * the loads of NS_K rows are issued a chunk ahead into the second of two register buffers, then the current chunk's row steps run,
//     then its stores.  Loads and stores share vmcnt on gfx950: chunk c + 1's loads are issued BEFORE chunk c's stores, and no load sits
//     behind a branch -- rows below 0 are clamped to row 0 (loaded again, never used);
//   * NS_K = 16: a row is one byte load and one store.  When the wave waits for chunk c + 1's loads, what it has issued after them is
//     chunk c's stores and chunk c + 2's loads, 16 * (1 + 1) = 32 operations, which the six-bit vmcnt (63) counts exactly;
//   * the address is a running pointer stepped in place by a wave-uniform stride; the flag bytes are held as they arrive.
//
// phx_nstep_fold_kernel: fully parallel over the T * N elements, a thread per element, consecutive lanes on consecutive columns of one
// row.  A thread at a trajectory row walks at most n hops along succ_row (acted == NULL: t + 1): per hop it loads reward, the flag bytes,
// next_row and succ_row of the hop's row, and after its LAST load it stores its six outputs once: no load follows a store (3.2b for
// free).  A hop's five loads are issued together, ahead of every test, and pinned there (an empty asm that names the five values: left to
// itself the compiler masks a hole lane out of the loop and loads reward and succ_row only after the flags and next_row have said that
// the hop counts -- two dependent round trips per hop where one will do; the pinned form was not timed against the other).
// A hole row therefore loads what a trajectory row's first hop loads, and stores +0.0, +0.0, -1, 0, 0, -1.  A NULL input plane is a
// template parameter (terminated, acted, next_row: eight instantiations), so that no load sits behind a never-true condition.  The
// chain is the header's, operation for operation: the first reward assigned, then fmaf(p, r, G), p by repeated multiplication.  No LDS,
// no array.  The work is bounded by T * N * n hops; hops of neighbouring lanes at the same depth read neighbouring columns of nearby rows.
//
// phx_nstep_gather_kernel (only with nstep_next_obs): built as phx_traj_gather_kernel -- a thread owns one word of a row's N * D and
// NG_ROWS consecutive rows: it loads nstep_last of its rows, then the source word of each row unconditionally (the row clamped to 0 for
// -1) and selects.  Words are moved as 32-bit integers, never computed with; 32-bit index arithmetic where N * D fits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_nstep.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int NS_K = 16;           // rows per chunk of the succ scan (tests/test_gpu_nstep.py walks T below, at and across it)
constexpr int NS_LANES = 64;       // columns per workgroup of the succ scan: one wave
constexpr int NF_THREADS = 256;    // the fold's workgroup: 256 consecutive columns of a row
constexpr int NG_THREADS = 256;    // the gather's workgroup: 256 consecutive words of a row
constexpr int NG_ROWS = 4;         // rows per gather thread (the index arithmetic is paid once for them, their loads overlap)
constexpr int NSTEP_MAX_N = 64;

struct NsChunk {
  uint32_t ac[NS_K];
};

// the load stream of a column: `acted` at row `t` of the column, walked down a row at a time and held at row 0
struct NsStream {
  const uint8_t* ac;
  int t;
  __device__ __forceinline__ NsStream(const phx_nstep_io& a, const int64_t n) : ac(a.acted + ((int64_t)(a.T - 1) * a.N + n)), t(a.T - 1) {}
  __device__ __forceinline__ void down(const phx_nstep_io& a) {
    const int64_t step = t > 0 ? -a.N : 0;               // (wave-uniform)
    t = t > 0 ? t - 1 : 0;
    ac += step;
  }
};

// the next NS_K rows of the stream (rows below 0: row 0 again)
__device__ __forceinline__ void ns_load(NsChunk& c, const phx_nstep_io& a, NsStream& p) {
#pragma unroll
  for (int k = 0; k < NS_K; ++k) {
    c.ac[k] = *p.ac;
    p.down(a);
  }
}

// the chunk's rows that exist: succ_row[t] = the state, then the state becomes t at a trajectory row
__device__ __forceinline__ void ns_chain(const NsChunk& c, const phx_nstep_io& a, const int t_hi, int32_t& nx, int32_t*& out) {
#pragma unroll
  for (int k = 0; k < NS_K; ++k) {
    const int t = t_hi - k;
    if (t < 0) break;                                    // (wave-uniform, and around a store only)
    __builtin_nontemporal_store(nx, out);
    nx = c.ac[k] != 0 ? t : nx;
    out += -a.N;
  }
}

__global__ __launch_bounds__(NS_LANES) void phx_nstep_succ_kernel(const phx_nstep_io a) {
  const int64_t n = (int64_t)blockIdx.x * NS_LANES + threadIdx.x;
  if (n >= a.N) return;
  NsChunk c0, c1;
  NsStream p(a, n);
  int t_hi = a.T - 1;
  int32_t nx = -1;
  int32_t* out = a.succ_row + ((int64_t)t_hi * a.N + n);
  ns_load(c0, a, p);
  for (;;) {
    ns_load(c1, a, p);
    ns_chain(c0, a, t_hi, nx, out);
    t_hi -= NS_K;
    if (t_hi < 0) break;
    ns_load(c0, a, p);
    ns_chain(c1, a, t_hi, nx, out);
    t_hi -= NS_K;
    if (t_hi < 0) break;
  }
}

template <bool HAS_TERM, bool HAS_ACT, bool HAS_NR>
__global__ __launch_bounds__(NF_THREADS) void phx_nstep_fold_kernel(const phx_nstep_io a) {
  const int64_t n = (int64_t)blockIdx.x * NF_THREADS + threadIdx.x;
  if (n >= a.N) return;
  // (a row per workgroup row of the grid; the grid has at most 65535 of them: a longer fragment goes round)
  for (int t0 = (int)blockIdx.y; t0 < a.T; t0 += (int)gridDim.y) {
    const bool live = !HAS_ACT || a.acted[(int64_t)t0 * a.N + n] != 0;
    float G = 0.0f, p = 1.0f;
    int32_t u = t0, last = -1, nrow = -1;
    bool lterm = false, ltrunc = false;
    for (int m = 0;;) {                                  // the header's loop; u is a row of the fragment in every pass
      const int64_t e = (int64_t)u * a.N + n;
      float r = a.reward[e];
      uint32_t tr = a.truncated[e];
      uint32_t te = HAS_TERM ? a.terminated[e] : 0u;
      int32_t nr = HAS_NR ? a.next_row[e] : u;
      int32_t su = HAS_ACT ? a.succ_row[e] : (u + 1 < a.T ? u + 1 : -1);
      asm volatile("" : "+v"(r), "+v"(tr), "+v"(te), "+v"(nr), "+v"(su));      // the hop's loads stay together, ahead of every test (phx_vtrace.hip's idiom)
      if (!live) break;                                  // (a hole row: it loaded what a trajectory row loads)
      const bool term = te != 0;
      const bool trunc = !term && tr != 0;
      const bool cmp = term || trunc || nr >= 0;         // (next_row == NULL: nr = u >= 0)
      if (m > 0 && !cmp) break;
      G = m == 0 ? r : __builtin_fmaf(p, r, G);
      last = u;
      lterm = term;
      ltrunc = trunc;
      nrow = nr;
      m += 1;
      p = p * a.gamma;
      if (!cmp || term || trunc || m == a.n) break;
      u = su;
      if (u < 0) break;
    }
    const int64_t e0 = (int64_t)t0 * a.N + n;
    __builtin_nontemporal_store(live ? G : 0.0f, a.nstep_reward + e0);
    __builtin_nontemporal_store(live ? p : 0.0f, a.nstep_discount + e0);
    __builtin_nontemporal_store(last, a.nstep_last + e0);
    __builtin_nontemporal_store((uint8_t)(lterm ? 1 : 0), a.nstep_terminated + e0);
    __builtin_nontemporal_store((uint8_t)(ltrunc ? 1 : 0), a.nstep_truncated + e0);
    __builtin_nontemporal_store(nrow, a.nstep_next_row + e0);
  }
}

// nstep_next_obs: word w of row t is word d = w % D of column n = w / D.  IDX: 32-bit where N * D fits (the division is then a short one)
template <typename IDX>
__global__ __launch_bounds__(NG_THREADS) void phx_nstep_gather_kernel(const phx_nstep_io a, const IDX row_words) {
  const IDX w = (IDX)blockIdx.x * NG_THREADS + threadIdx.x;
  if (w >= row_words) return;
  const IDX n = w / (IDX)a.D;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.next_obs);
  uint32_t* out = reinterpret_cast<uint32_t*>(a.nstep_next_obs);
  const int64_t rw = (int64_t)row_words;
  // (groups of NG_ROWS rows, one per workgroup row of the grid; the grid has at most 65535 of them: a longer fragment goes round)
  for (int64_t t0 = (int64_t)blockIdx.y * NG_ROWS; t0 < a.T; t0 += (int64_t)gridDim.y * NG_ROWS) {
    int32_t la[NG_ROWS];
    uint32_t got[NG_ROWS];
#pragma unroll
    for (int r = 0; r < NG_ROWS; ++r) {                  // (rows past the fragment's last: row T - 1 again, never stored)
      const int64_t t = t0 + r < a.T ? t0 + r : a.T - 1;
      la[r] = a.nstep_last[t * a.N + (int64_t)n];
    }
#pragma unroll
    for (int r = 0; r < NG_ROWS; ++r) {
      const int64_t s = la[r] < 0 ? 0 : la[r];           // (-1: row 0 is loaded and not selected; the fold wrote nstep_last < T)
      got[r] = src[s * rw + (int64_t)w];
    }
#pragma unroll
    for (int r = 0; r < NG_ROWS; ++r) {
      const int64_t t = t0 + r;
      if (t >= a.T) break;                               // (uniform, and around a store only)
      __builtin_nontemporal_store(la[r] >= 0 ? got[r] : 0u, out + (t * rw + (int64_t)w));
    }
  }
}

// instantiation W: bit 2 terminated, bit 1 acted, bit 0 next_row given
template <int W>
static void nf_launch(const int which, const phx_nstep_io& io, hipStream_t st) {
  if (which == W) {
    const dim3 grid((unsigned)((io.N + NF_THREADS - 1) / NF_THREADS), (unsigned)min(io.T, 65535));
    hipLaunchKernelGGL((phx_nstep_fold_kernel<(W & 4) != 0, (W & 2) != 0, (W & 1) != 0>), grid, dim3(NF_THREADS), 0, st, io);
  } else if constexpr (W > 0) {
    nf_launch<W - 1>(which, io, st);
  }
}

template <typename IDX>
static void ng_launch(const phx_nstep_io& io, hipStream_t st) {
  const int64_t row_words = io.N * io.D;
  const dim3 grid((unsigned)((row_words + NG_THREADS - 1) / NG_THREADS), (unsigned)min((io.T + NG_ROWS - 1) / NG_ROWS, 65535));
  hipLaunchKernelGGL((phx_nstep_gather_kernel<IDX>), grid, dim3(NG_THREADS), 0, st, io, (IDX)row_words);
}

extern "C" int phx_nstep(const phx_nstep_io* io, void* stream) {
  const char* fn = "phx_nstep";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, NS_LANES)) return rc;
  if (io->n < 1 || io->n > NSTEP_MAX_N) return fail(PHX_EINVAL, "phx_nstep: n = %d must lie in [1, %d]", io->n, NSTEP_MAX_N);
  if (!frag_unit(io->gamma)) return fail(PHX_EINVAL, "phx_nstep: gamma = %g must lie in [0, 1]", (double)io->gamma);
  if (const int rc = frag_required(fn, io->reward && io->truncated, "reward and truncated")) return rc;
  if (const int rc = frag_required(fn, io->nstep_reward && io->nstep_discount && io->nstep_last && io->nstep_terminated && io->nstep_truncated &&
                                           io->nstep_next_row,
                                   "nstep_reward, nstep_discount, nstep_last, nstep_terminated, nstep_truncated and nstep_next_row"))
    return rc;
  if (io->acted && !io->succ_row) return fail(PHX_EINVAL, "phx_nstep: acted needs succ_row");
  if (io->nstep_next_obs) {
    if (!io->next_obs) return fail(PHX_EINVAL, "phx_nstep: nstep_next_obs needs next_obs");
    if (io->D < 1 || io->D > 64) return fail(PHX_EINVAL, "phx_nstep: D = %d must lie in [1, 64] when nstep_next_obs is given", io->D);
    if (io->N * io->D > (int64_t)NG_THREADS * 0x7fffffff) return frag_beyond_grid(fn, "N = %lld with D = %d is", (long long)io->N, io->D);
  }
  if (const int rc = frag_aligned(fn, frag_bits(io->reward, io->next_row, io->next_obs), 4, "reward, next_row and next_obs")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->succ_row, io->nstep_reward, io->nstep_discount, io->nstep_last, io->nstep_terminated,
                                                io->nstep_truncated, io->nstep_next_row, io->nstep_next_obs),
                                  16, "succ_row and the nstep_ outputs"))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  if (io->acted) {
    hipLaunchKernelGGL(phx_nstep_succ_kernel, dim3((unsigned)((io->N + NS_LANES - 1) / NS_LANES)), dim3(NS_LANES), 0, st, *io);
    if (const int rc = call.launched("the successor scan", "phx_nstep_succ_kernel")) return rc;
  }
  const int which = (io->terminated ? 4 : 0) | (io->acted ? 2 : 0) | (io->next_row ? 1 : 0);
  nf_launch<7>(which, *io, st);
  if (const int rc = call.launched("the fold", "phx_nstep_fold_kernel")) return rc;
  if (io->nstep_next_obs) {
    if (io->N * io->D <= 0xffffff00LL) ng_launch<uint32_t>(*io, st); else ng_launch<uint64_t>(*io, st);
    if (const int rc = call.launched("the gather", "phx_nstep_gather_kernel")) return rc;
  }
  return PHX_OK;
}
