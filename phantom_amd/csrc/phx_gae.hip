// phx_gae.hip -- phx_gae (include/phantom_amd_gae.h): advantages and value targets of a rollout fragment in one launch.
//
// The recurrence runs backwards over the T rows of a column and is two fmaf and two adds per element: the kernel streams
// its planes once and is bound by memory, within a column by load latency.  No load depends on the chain, so:
//   * a lane owns ONE column and a wave 64 consecutive ones: every row access of a wave is one coalesced 256-byte (f32) or
//     64-byte (u8) piece, at any alignment of the input planes and for any N (lanes past N leave at entry).  One wave per
//     workgroup, so that the 576 waves of N = 36 864 spread over the chip's 1 024 SIMDs;
//   * with less than a wave per SIMD, the bytes in flight come from depth: the loads of GAE_K rows are issued a chunk ahead
//     into the second of two register buffers, then the chain of the current chunk runs, then its stores.  Loads and stores
//     share vmcnt on gfx950: the next chunk's loads are issued BEFORE this chunk's stores, and no load sits
//     behind a branch -- rows past the fragment's first are clamped to row 0 (loaded again, never used);
//   * vf_next is loaded with the chunk, unconditionally: a select, not arithmetic, discards the rows the definition does
//     not read (what was measured against loading only the rows a wave's ballot asks for: DESIGN 3.4e);
//   * the outputs are never read again: non-temporal stores, as the store-wave rollout kernel's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_gae.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int GAE_K = 16;          // rows per chunk (tests/test_gpu_gae.py walks T below, at and across it)
constexpr int GAE_LANES = 64;      // columns per workgroup: one wave

template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM>
struct GaeChunk {
  float r[GAE_K], v[HAS_V ? GAE_K : 1], vn[HAS_NEXT ? GAE_K : 1];
  uint32_t tr[GAE_K], te[HAS_TERM ? GAE_K : 1];
};

// rows t_hi, t_hi - 1 .. t_hi - GAE_K + 1 of column n (rows below 0: row 0 again)
template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM>
__device__ __forceinline__ void gae_load(GaeChunk<HAS_V, HAS_NEXT, HAS_TERM>& c, const phx_gae_io& a, const int64_t n, const int t_hi) {
#pragma unroll
  for (int k = 0; k < GAE_K; ++k) {
    const int t = t_hi - k > 0 ? t_hi - k : 0;
    const int64_t o = (int64_t)t * a.N + n;
    c.r[k] = a.reward[o];
    if (HAS_V) c.v[k] = a.vf_pred[o];
    if (HAS_NEXT) c.vn[k] = a.vf_next[o];
    c.tr[k] = a.truncated[o];
    if (HAS_TERM) c.te[k] = a.terminated[o];
  }
}

// the definition for the chunk's rows that exist; adv_next / v_next: advantage[t + 1][n] and vf_pred[t + 1][n] on entry and exit
template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM>
__device__ __forceinline__ void gae_chain(const GaeChunk<HAS_V, HAS_NEXT, HAS_TERM>& c, const phx_gae_io& a, const float gl, const int64_t n,
                                          const int t_hi, float& adv_next, float& v_next) {
#pragma unroll
  for (int k = 0; k < GAE_K; ++k) {
    const int t = t_hi - k;
    if (t < 0) break;                                    // (wave-uniform, and around stores only)
    const int64_t o = (int64_t)t * a.N + n;
    const bool term = HAS_TERM && c.te[k] != 0;
    const bool cut = term || c.tr[k] != 0 || t == a.T - 1;
    const float v = HAS_V ? c.v[k] : 0.0f;
    const float nv = term ? 0.0f : (cut ? (HAS_NEXT ? c.vn[k] : 0.0f) : v_next);
    const float cc = cut ? 0.0f : adv_next;
    const float d = __builtin_fmaf(a.gamma, nv, c.r[k]) - v;
    const float adv = __builtin_fmaf(gl, cc, d);
    __builtin_nontemporal_store(adv, a.advantage + o);
    if (a.value_target) __builtin_nontemporal_store(adv + v, a.value_target + o);
    adv_next = adv;
    v_next = v;
  }
}

template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM>
__global__ __launch_bounds__(GAE_LANES) void phx_gae_kernel(const phx_gae_io a, const float gl) {
  const int64_t n = (int64_t)blockIdx.x * GAE_LANES + threadIdx.x;
  if (n >= a.N) return;
  GaeChunk<HAS_V, HAS_NEXT, HAS_TERM> c0, c1;
  float adv_next = 0.0f, v_next = 0.0f;                  // (never used at t == T - 1: the row is a cut)
  int t_hi = a.T - 1;
  gae_load(c0, a, n, t_hi);
  for (;;) {
    gae_load(c1, a, n, t_hi - GAE_K);
    gae_chain(c0, a, gl, n, t_hi, adv_next, v_next);
    t_hi -= GAE_K;
    if (t_hi < 0) break;
    gae_load(c0, a, n, t_hi - GAE_K);
    gae_chain(c1, a, gl, n, t_hi, adv_next, v_next);
    t_hi -= GAE_K;
    if (t_hi < 0) break;
  }
}

template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM>
static void gae_launch(const phx_gae_io& io, const float gl, hipStream_t st) {
  const unsigned grid = (unsigned)((io.N + GAE_LANES - 1) / GAE_LANES);
  hipLaunchKernelGGL((phx_gae_kernel<HAS_V, HAS_NEXT, HAS_TERM>), dim3(grid), dim3(GAE_LANES), 0, st, io, gl);
}

extern "C" int phx_gae(const phx_gae_io* io, void* stream) {
  const char* fn = "phx_gae";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_reserved0(fn, io->reserved0)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, GAE_LANES)) return rc;
  if (const int rc = frag_gamma_lambda(fn, io->gamma, io->lambda)) return rc;
  if (const int rc = frag_required(fn, io->reward && io->truncated && io->advantage, "reward, truncated and advantage")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->reward, io->vf_pred, io->vf_next), 4, "reward, vf_pred and vf_next")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->advantage, io->value_target), 16, "advantage and value_target")) return rc;
  const float gl = io->gamma * io->lambda;               // one f32 multiply (the build has -ffp-contract=off)
  const hipStream_t st = (hipStream_t)stream;
  const int which = (io->vf_pred ? 4 : 0) | (io->vf_next ? 2 : 0) | (io->terminated ? 1 : 0);
  switch (which) {
    case 0: gae_launch<false, false, false>(*io, gl, st); break;
    case 1: gae_launch<false, false, true>(*io, gl, st); break;
    case 2: gae_launch<false, true, false>(*io, gl, st); break;
    case 3: gae_launch<false, true, true>(*io, gl, st); break;
    case 4: gae_launch<true, false, false>(*io, gl, st); break;
    case 5: gae_launch<true, false, true>(*io, gl, st); break;
    case 6: gae_launch<true, true, false>(*io, gl, st); break;
    default: gae_launch<true, true, true>(*io, gl, st); break;
  }
  return FragCall{fn}.launched(nullptr, "phx_gae_kernel");
}
