// phx_vtrace.hip -- phx_vtrace (include/phantom_amd_vtrace.h): V-trace value targets and policy-gradient advantages of a rollout
// fragment in one launch.
//
// The same reverse scan over the T rows of a column as phx_gae_kernel (phx_gae.hip, which this file leaves alone), over two more f32
// planes -- the two log-densities -- and with two coupled recurrences.  The mapping and the discipline are phx_gae_kernel's
// (what differs: DESIGN 3.4g):
//   * a lane owns ONE column and a wave 64 consecutive ones, one wave per workgroup: every row access of a wave is one coalesced
//     256-byte (f32) or 64-byte (u8) piece at any alignment of the inputs and for any N (lanes past N leave at entry);
//   * the loads of VT_K rows are issued a chunk ahead into the second of two register buffers, then the current chunk is computed,
//     then stored.  Loads and stores share vmcnt on gfx950: the next chunk's loads are issued BEFORE this chunk's stores, and no load
//     sits behind a branch -- rows past the fragment's first are clamped to row 0 (loaded again, never used), a NULL input plane is a
//     template parameter (vf_next, terminated: four instantiations), pg_advantage == NULL a uniform branch around a store;
//   * VT_K = 8, not 16: a chunk is 56 loads (8 rows x five f32 planes and two flag bytes), which the 63 a wave can have outstanding
//     (vmcnt is six bits) still count exactly -- at 16 rows the wait for the current chunk also waits for most of the next one -- and
//     the two buffers, the weights and the pointers below fit 153 registers: three waves per SIMD where 16 rows leave two or one;
//   * addresses are running pointers, one per plane, stepped in place by a wave-uniform stride (VtStream): the load phase then holds
//     no wait at all.  Formed per row from (t, n), the 64-bit addresses go through temporaries that the register allocator places in
//     registers a load in flight still writes, and the compiler waits for that load before it issues the next one;
//   * the loaded values are held as they arrive: the log-ratio is NOT formed in the load phase (an operation on a loaded value
//     there is a wait, which the two buffers exist to avoid);
//   * the exp is OFF the recurrence.  rho and the three clipped weights of a row depend on nothing carried: vt_weights computes them
//     for all VT_K rows of the chunk first -- VT_K independent chains of about a dozen dependent operations, which overlap -- and the
//     carried chain that follows is one multiply and one fmaf per row, plus the pg_advantage side chain through vs[t + 1];
//   * the outputs are never read again: non-temporal stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_vtrace.h"
#include "phx_sc_policy.h"         // pol_exp: the PHX_EXP_* procedure of phantom_amd.h (device inlines only, no kernel)
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int VT_K = 8;            // rows per chunk (tests/test_gpu_vtrace.py walks T below, at and across it)
constexpr int VT_LANES = 64;       // columns per workgroup: one wave

template <bool HAS_NEXT, bool HAS_TERM>
struct VtChunk {
  float r[VT_K], v[VT_K], bl[VT_K], tl[VT_K], vn[HAS_NEXT ? VT_K : 1];
  uint32_t tr[VT_K], te[HAS_TERM ? VT_K : 1];
};

// the clipped importance weights of the chunk's rows (the header's rc, gc, rp)
struct VtWeights {
  float rc[VT_K], gc[VT_K], rp[VT_K];
};

// the load stream of a column: one pointer per input plane at row `t` of the column, walked down a row at a time and held at row 0.  The
// pointers are updated in place (one 64-bit add of a wave-uniform stride per load) and live for the whole kernel, so no address is
// formed in a temporary register -- which the register allocator otherwise places where a load in flight still writes, with a wait each
template <bool HAS_NEXT, bool HAS_TERM>
struct VtStream {
  const float *r, *v, *bl, *tl, *vn;
  const uint8_t *tr, *te;
  int t;
  __device__ __forceinline__ VtStream(const phx_vtrace_io& a, const int64_t n) : t(a.T - 1) {
    const int64_t o = (int64_t)t * a.N + n;
    r = a.reward + o; v = a.vf_pred + o; bl = a.behaviour_logp + o; tl = a.target_logp + o; tr = a.truncated + o;
    vn = HAS_NEXT ? a.vf_next + o : nullptr;
    te = HAS_TERM ? a.terminated + o : nullptr;
  }
  __device__ __forceinline__ void down(const phx_vtrace_io& a) {
    const int64_t step = t > 0 ? -a.N : 0;               // (wave-uniform; added: one v_lshl_add_u64 per pointer)
    t = t > 0 ? t - 1 : 0;
    r += step; v += step; bl += step; tl += step; tr += step;
    if (HAS_NEXT) vn += step;
    if (HAS_TERM) te += step;
  }
};

// the next VT_K rows of the stream (rows below 0: row 0 again)
template <bool HAS_NEXT, bool HAS_TERM>
__device__ __forceinline__ void vt_load(VtChunk<HAS_NEXT, HAS_TERM>& c, const phx_vtrace_io& a, VtStream<HAS_NEXT, HAS_TERM>& p) {
#pragma unroll
  for (int k = 0; k < VT_K; ++k) {
    c.r[k] = *p.r;
    c.v[k] = *p.v;
    c.bl[k] = *p.bl;
    c.tl[k] = *p.tl;
    if (HAS_NEXT) c.vn[k] = *p.vn;
    c.tr[k] = *p.tr;
    if (HAS_TERM) c.te[k] = *p.te;
    p.down(a);
  }
}

// per element, independent of the scan: VT_K independent chains (clamped rows compute row 0's weights again, never used)
template <bool HAS_NEXT, bool HAS_TERM>
__device__ __forceinline__ void vt_weights(const VtChunk<HAS_NEXT, HAS_TERM>& c, const phx_vtrace_io& a, VtWeights& w) {
#pragma unroll
  for (int k = 0; k < VT_K; ++k) {
    const float lr = __fsub_rn(c.tl[k], c.bl[k]);
    const float l = lr < PHX_LOG_STD_MIN ? PHX_LOG_STD_MIN : (lr > PHX_LOG_STD_MAX ? PHX_LOG_STD_MAX : lr);      // (-20, 20: the domain of pol_exp)
    const float rho = pol_exp(l);
    w.rc[k] = rho < a.rho_bar ? rho : a.rho_bar;
    w.gc[k] = __fmul_rn(a.gamma, __fmul_rn(a.lambda, rho < a.c_bar ? rho : a.c_bar));
    w.rp[k] = rho < a.pg_rho_bar ? rho : a.pg_rho_bar;
  }
  // (the three weights of every row exist HERE, in registers: without this the compiler sinks each row's exp into the row's block of the
  //  carried chain below, behind its `t < 0` branch, where the chains no longer overlap)
#pragma unroll
  for (int k = 0; k < VT_K; ++k) asm volatile("" : "+v"(w.rc[k]), "+v"(w.gc[k]), "+v"(w.rp[k]));
}

// what a column carries from row t + 1 to row t (never used at t == T - 1: the row is a cut)
struct VtState {
  float acc = 0.0f, vs_next = 0.0f, v_next = 0.0f;
  float *vs_out, *pg_out;                                // the column's elements of the two output planes at the row the chain is at
};

// the definition's scan for the chunk's rows that exist
template <bool HAS_NEXT, bool HAS_TERM>
__device__ __forceinline__ void vt_chain(const VtChunk<HAS_NEXT, HAS_TERM>& c, const VtWeights& w, const phx_vtrace_io& a, const int t_hi,
                                         VtState& s) {
#pragma unroll
  for (int k = 0; k < VT_K; ++k) {
    const int t = t_hi - k;
    if (t < 0) break;                                    // (wave-uniform, and around stores only)
    const bool term = HAS_TERM && c.te[k] != 0;
    const bool cut = term || c.tr[k] != 0 || t == a.T - 1;
    const float v = c.v[k];
    const float boot = HAS_NEXT ? c.vn[k] : 0.0f;
    const float nv = term ? 0.0f : (cut ? boot : s.v_next);
    const float nvs = term ? 0.0f : (cut ? boot : s.vs_next);
    const float cc = cut ? 0.0f : s.acc;
    const float td = __fsub_rn(__fmaf_rn(a.gamma, nv, c.r[k]), v);
    s.acc = __fmaf_rn(w.gc[k], cc, __fmul_rn(w.rc[k], td));
    const float vs = __fadd_rn(s.acc, v);
    __builtin_nontemporal_store(vs, s.vs_out);
    if (a.pg_advantage) __builtin_nontemporal_store(__fmul_rn(w.rp[k], __fsub_rn(__fmaf_rn(a.gamma, nvs, c.r[k]), v)), s.pg_out);
    s.vs_next = vs;
    s.v_next = v;
    s.vs_out += -a.N;
    s.pg_out += -a.N;
  }
}

template <bool HAS_NEXT, bool HAS_TERM>
__global__ __launch_bounds__(VT_LANES) void phx_vtrace_kernel(const phx_vtrace_io a) {
  const int64_t n = (int64_t)blockIdx.x * VT_LANES + threadIdx.x;
  if (n >= a.N) return;
  VtChunk<HAS_NEXT, HAS_TERM> c0, c1;
  VtWeights w;
  VtStream<HAS_NEXT, HAS_TERM> p(a, n);
  VtState s;
  int t_hi = a.T - 1;
  s.vs_out = a.vs + ((int64_t)t_hi * a.N + n);
  s.pg_out = a.pg_advantage + ((int64_t)t_hi * a.N + n);  // (never dereferenced when pg_advantage is NULL)
  vt_load(c0, a, p);
  for (;;) {
    vt_load(c1, a, p);
    vt_weights(c0, a, w);
    vt_chain(c0, w, a, t_hi, s);
    t_hi -= VT_K;
    if (t_hi < 0) break;
    vt_load(c0, a, p);
    vt_weights(c1, a, w);
    vt_chain(c1, w, a, t_hi, s);
    t_hi -= VT_K;
    if (t_hi < 0) break;
  }
}

template <bool HAS_NEXT, bool HAS_TERM>
static void vt_launch(const phx_vtrace_io& io, hipStream_t st) {
  const unsigned grid = (unsigned)((io.N + VT_LANES - 1) / VT_LANES);
  hipLaunchKernelGGL((phx_vtrace_kernel<HAS_NEXT, HAS_TERM>), dim3(grid), dim3(VT_LANES), 0, st, io);
}

static bool vt_threshold_ok(const float x) { return x > 0.0f && x <= 3.402823466e+38f; }      // finite and > 0 (NaN fails both)

extern "C" int phx_vtrace(const phx_vtrace_io* io, void* stream) {
  const char* fn = "phx_vtrace";
  if (const int rc = frag_io(fn, io)) return rc;
  if (io->reserved0 != 0 || !(io->reserved1 == 0.0f)) return fail(PHX_EINVAL, "phx_vtrace: reserved0 and reserved1 must be 0");
  if (const int rc = frag_rows_cols(fn, io->T, io->N)) return rc;
  if (const int rc = frag_one_grid(fn, "N", io->N, VT_LANES)) return rc;
  if (const int rc = frag_gamma_lambda(fn, io->gamma, io->lambda)) return rc;
  if (!vt_threshold_ok(io->rho_bar) || !vt_threshold_ok(io->c_bar) || !vt_threshold_ok(io->pg_rho_bar))
    return fail(PHX_EINVAL, "phx_vtrace: rho_bar = %g, c_bar = %g and pg_rho_bar = %g must be finite and > 0", (double)io->rho_bar,
                (double)io->c_bar, (double)io->pg_rho_bar);
  if (const int rc = frag_required(fn, io->reward && io->vf_pred && io->behaviour_logp && io->target_logp && io->truncated && io->vs,
                                   "reward, vf_pred, behaviour_logp, target_logp, truncated and vs"))
    return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->reward, io->vf_pred, io->vf_next, io->behaviour_logp, io->target_logp), 4,
                                  "reward, vf_pred, vf_next, behaviour_logp and target_logp"))
    return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->vs, io->pg_advantage), 16, "vs and pg_advantage")) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int which = (io->vf_next ? 2 : 0) | (io->terminated ? 1 : 0);
  switch (which) {
    case 0: vt_launch<false, false>(*io, st); break;
    case 1: vt_launch<false, true>(*io, st); break;
    case 2: vt_launch<true, false>(*io, st); break;
    default: vt_launch<true, true>(*io, st); break;
  }
  return FragCall{fn}.launched(nullptr, "phx_vtrace_kernel");
}
