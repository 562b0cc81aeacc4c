// phx_gae_masked.hip -- phx_gae_masked (include/phantom_amd_gae.h): advantages, value targets and per-action reward sums of a
// fragment whose per-agent trajectories have holes (FSM / Stackelberg envs: acted and reward_valid planes), in one launch.
//
// The same reverse scan over the T rows of a column as phx_gae_kernel (phx_gae.hip, which this file leaves alone), with a few
// more words of state per column: the running reward sum of the open segment, the bootstrap value of its closing cut row and
// three flags.  The mapping and the discipline are phx_gae_kernel's:
//   * a lane owns ONE column and a wave 64 consecutive ones, one wave per workgroup: every row access of a wave is one coalesced
//     256-byte (f32) or 64-byte (u8) piece at any alignment of the inputs and for any N (lanes past N leave at entry);
//   * the loads of GMK_K rows are issued a chunk ahead into the second of two register buffers, then the chain of the current
//     chunk runs, then its stores.  Loads and stores share vmcnt on gfx950: the next chunk's loads are issued BEFORE this chunk's
//     stores, and no load sits behind a branch -- rows past the fragment's first are clamped to row 0 (loaded again, never used),
//     a NULL plane is a template parameter (32 instantiations; a NULL output is a uniform branch around a store);
//   * the four flag bytes of a row are held as they arrive, one register each: packing them needs an operation on the loaded
//     value, which would put a wait into the load phase;
//   * the row step is selects only: a hole row computes what a trajectory row computes and stores three zeros, so that the
//     output planes are written everywhere.  Non-temporal stores: the outputs are never read again.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_gae.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int GMK_K = 16;          // rows per chunk (tests/test_gpu_gae_masked.py walks T below, at and across it)
constexpr int GMK_LANES = 64;      // columns per workgroup: one wave

template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
struct GmkChunk {
  float r[GMK_K], v[HAS_V ? GMK_K : 1], vn[HAS_NEXT ? GMK_K : 1];
  uint32_t tr[GMK_K], te[HAS_TERM ? GMK_K : 1], ac[HAS_ACT ? GMK_K : 1], rv[HAS_RV ? GMK_K : 1];
};

// what a column carries from row t + 1 to row t (the header's definition, same names)
struct GmkState {
  float acc = 0.0f, nv = 0.0f, adv_next = 0.0f, v_next = 0.0f;
  bool empty = true, cut = true, term = false;
};

// rows t_hi, t_hi - 1 .. t_hi - GMK_K + 1 of column n (rows below 0: row 0 again)
template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__device__ __forceinline__ void gmk_load(GmkChunk<HAS_V, HAS_NEXT, HAS_TERM, HAS_ACT, HAS_RV>& c, const phx_gae_masked_io& a, const int64_t n,
                                         const int t_hi) {
#pragma unroll
  for (int k = 0; k < GMK_K; ++k) {
    const int t = t_hi - k > 0 ? t_hi - k : 0;
    const int64_t o = (int64_t)t * a.N + n;
    c.r[k] = a.reward[o];
    if (HAS_V) c.v[k] = a.vf_pred[o];
    if (HAS_NEXT) c.vn[k] = a.vf_next[o];
    c.tr[k] = a.truncated[o];
    if (HAS_TERM) c.te[k] = a.terminated[o];
    if (HAS_ACT) c.ac[k] = a.acted[o];
    if (HAS_RV) c.rv[k] = a.reward_valid[o];
  }
}

// the definition for the chunk's rows that exist
template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__device__ __forceinline__ void gmk_chain(const GmkChunk<HAS_V, HAS_NEXT, HAS_TERM, HAS_ACT, HAS_RV>& c, const phx_gae_masked_io& a, const float gl,
                                          const int64_t n, const int t_hi, GmkState& s) {
#pragma unroll
  for (int k = 0; k < GMK_K; ++k) {
    const int t = t_hi - k;
    if (t < 0) break;                                    // (wave-uniform, and around stores only)
    const int64_t o = (int64_t)t * a.N + n;
    const bool te = HAS_TERM && c.te[k] != 0;
    const bool crow = te || c.tr[k] != 0 || t == a.T - 1;
    s.empty = crow || s.empty;
    s.cut = crow || s.cut;
    s.term = crow ? te : s.term;
    s.nv = crow ? (te || !HAS_NEXT ? 0.0f : c.vn[k]) : s.nv;
    const bool present = !HAS_RV || c.rv[k] == 1;
    s.acc = present ? (s.empty ? c.r[k] : c.r[k] + s.acc) : s.acc;
    s.empty = s.empty && !present;
    const bool act = !HAS_ACT || c.ac[k] != 0;
    const float rs = s.empty ? 0.0f : s.acc;
    const float v = HAS_V ? c.v[k] : 0.0f;
    const float nvv = s.term ? 0.0f : (s.cut ? s.nv : s.v_next);
    const float cc = s.cut ? 0.0f : s.adv_next;
    const float d = __builtin_fmaf(a.gamma, nvv, rs) - v;
    const float adv = __builtin_fmaf(gl, cc, d);
    __builtin_nontemporal_store(act ? adv : 0.0f, a.advantage + o);
    if (a.value_target) __builtin_nontemporal_store(act ? adv + v : 0.0f, a.value_target + o);
    if (a.reward_sum) __builtin_nontemporal_store(act ? rs : 0.0f, a.reward_sum + o);
    s.adv_next = act ? adv : s.adv_next;
    s.v_next = act ? v : s.v_next;
    s.empty = act || s.empty;
    s.cut = s.cut && !act;
    s.term = s.term && !act;
  }
}

template <bool HAS_V, bool HAS_NEXT, bool HAS_TERM, bool HAS_ACT, bool HAS_RV>
__global__ __launch_bounds__(GMK_LANES) void phx_gae_masked_kernel(const phx_gae_masked_io a, const float gl) {
  const int64_t n = (int64_t)blockIdx.x * GMK_LANES + threadIdx.x;
  if (n >= a.N) return;
  GmkChunk<HAS_V, HAS_NEXT, HAS_TERM, HAS_ACT, HAS_RV> c0, c1;
  GmkState s;
  int t_hi = a.T - 1;
  gmk_load(c0, a, n, t_hi);
  for (;;) {
    gmk_load(c1, a, n, t_hi - GMK_K);
    gmk_chain(c0, a, gl, n, t_hi, s);
    t_hi -= GMK_K;
    if (t_hi < 0) break;
    gmk_load(c0, a, n, t_hi - GMK_K);
    gmk_chain(c1, a, gl, n, t_hi, s);
    t_hi -= GMK_K;
    if (t_hi < 0) break;
  }
}

// instantiation W: bit 4 vf_pred, bit 3 vf_next, bit 2 terminated, bit 1 acted, bit 0 reward_valid given
template <int W>
static void gmk_launch(const int which, const phx_gae_masked_io& io, const float gl, hipStream_t st) {
  if (which == W) {
    const unsigned grid = (unsigned)((io.N + GMK_LANES - 1) / GMK_LANES);
    hipLaunchKernelGGL((phx_gae_masked_kernel<(W & 16) != 0, (W & 8) != 0, (W & 4) != 0, (W & 2) != 0, (W & 1) != 0>), dim3(grid), dim3(GMK_LANES),
                       0, st, io, gl);
  } else if constexpr (W > 0) {
    gmk_launch<W - 1>(which, io, gl, st);
  }
}

extern "C" int phx_gae_masked(const phx_gae_masked_io* io, void* stream) {
  const char* fn = "phx_gae_masked";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_reserved0(fn, io->reserved0)) return rc;
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, GMK_LANES)) return rc;
  if (const int rc = frag_gamma_lambda(fn, io->gamma, io->lambda)) return rc;
  if (const int rc = frag_required(fn, io->reward && io->truncated && io->advantage, "reward, truncated and advantage")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->reward, io->vf_pred, io->vf_next), 4, "reward, vf_pred and vf_next")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->advantage, io->value_target, io->reward_sum), 16, "advantage, value_target and reward_sum"))
    return rc;
  const float gl = io->gamma * io->lambda;               // one f32 multiply (the build has -ffp-contract=off)
  const int which = (io->vf_pred ? 16 : 0) | (io->vf_next ? 8 : 0) | (io->terminated ? 4 : 0) | (io->acted ? 2 : 0) | (io->reward_valid ? 1 : 0);
  gmk_launch<31>(which, *io, gl, (hipStream_t)stream);
  return FragCall{fn}.launched(nullptr, "phx_gae_masked_kernel");
}
