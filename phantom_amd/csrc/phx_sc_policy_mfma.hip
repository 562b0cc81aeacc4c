// phx_sc_policy_mfma.hip -- the fused supply-chain rollout with a device policy (phx_rollout_io.policy) for networks of RLlib's default
// size: hidden layers up to 256 units, tanh (fcnet_hiddens = [256, 256], fcnet_activation = "tanh").
//
// Same env semantics as phx_sc_rollout_policy_kernel (phx_sc_policy.hip; the row's state and step are phx_sc_policy.h's): the policy on
// the previous observation (the reset observation after an episode's last step), decode_action, device Philox orders or replayed `exo`,
// the closed-form step, the trajectory row, auto-reset, last_obs.  What differs is who evaluates the network: a workgroup of four waves
// evaluates it for NR = 64 (S <= 64) or 128 rows (env, shop) at a time, one step after the other:
//   * layer 0 (K = 3) on VALU: every lane one row and a quarter (NR = 64) or half (NR = 128) of the units; act(c) into an LDS image
//     h[unit][row] (the rows of odd units rotated by 32, so that the two lane halves of an MFMA operand read hit different banks);
//   * layer 1 (two hidden layers) on f32 MFMA, v_mfma_f32_32x32x2_f32: D[unit][row] = C + W1[unit][k] h0[k][row] as ONE k-ascending
//     fmaf chain from C (gfx950: one rounding per product, no wider internal accumulation), with C = the bias and the k-steps of each
//     accumulator issued in ascending order -- the header's definition, bit for bit.  Wave w owns the 32-unit blocks w and w + 4 and all
//     NR rows (2 or 4 32-row tiles): every weight fragment feeds 2 or 4 MFMAs, every activation fragment 1 or 2.  The weights do not fit
//     LDS (256 KB at 256 x 256) and stream from L2 every step, 16 bytes per lane (torch's [W1][W0] rows, four k at a time) four k-pairs
//     ahead of their MFMAs; the activation fragments come from the LDS image; act() on VALU, back into the image (after a barrier: the
//     image is the input of the layer too);
//   * the output layer (one unit) on VALU: the lane of the row walks k ascending over the image (a 1-unit MFMA would be 31/32 zeros);
//   * padding: widths are rounded up to 32 with zero weights, zero biases and so zero activations (act(0) = 0 for all three): fmaf(0, 0, c)
//     = c changes at most the sign of an exact zero, which the definition's closing "+ 0.0f" removes from the action.
// A workgroup holds WHOLE envs (floor(NR / S) of them): an env's step counter and tick are read and written by one workgroup only.  The
// weight loads of a step wait behind the previous step's trajectory stores (vmcnt is shared): the stores leave three barriers
// and one layer before the first weight load that waits.
#include "phx_sc_policy.h"

#include <cstring>

typedef float mfma_f16 __attribute__((ext_vector_type(16)));

static const int MF_NT = 256;                    // four waves

// LDS (floats): [0, 4 W0p) layer 0 per unit (w0, w1, w2, b); b1 [W1p]; the output row [WLp] + its bias (+ 3 pad); x [NR][4]; h [Wmax][NR]
struct MfLayout { int w0, b1, wl, x, h, total; };
__host__ __device__ inline MfLayout mf_layout(int two, int W0p, int W1p, int NR) {
  MfLayout L;
  const int WLp = two ? W1p : W0p, Wmax = W0p > W1p ? W0p : W1p;
  L.w0 = 0; L.b1 = 4 * W0p; L.wl = L.b1 + (two ? W1p : 0); L.x = L.wl + WLp + 4; L.h = L.x + 4 * NR; L.total = L.h + Wmax * NR;
  return L;
}

// the image's index of unit u, row r
template <int NR>
__device__ __forceinline__ int mf_hidx(int u, int r) { return u * NR + (r ^ ((u & 1) << 5)); }

// ACT: PHX_ACT_*; TWO: two hidden layers; EXO: replayed order sizes; NR: rows per workgroup (64 or 128); VEC: W0 % 4 == 0 and w[1] 16-byte
// aligned (one 16-byte load per lane and four k; otherwise four guarded 4-byte loads)
// EXPLORE (phx_policy_explore, A = PolArgsX): a second output row, the head's log-std row [WLp] (zero where w_log_std is NULL) and its
// bias (+ 3 pad), after the layout's end; the output layer accumulates it beside y from the same image reads.  The step's noise is loaded
// one step ahead, before the row's trajectory stores.  One template body: phx_sc_rollout_policy_mfma_kernel instantiates it with EXPLORE =
// false, phx_sc_rollout_policy_mfma_explore_kernel with true.
template <int ACT, bool TWO, bool EXO, int NR, bool VEC, bool EXPLORE, class A>
__device__ __forceinline__ void pol_rollout_mfma(const A& a) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  constexpr int NTILE = NR / 32;                 // 32-row tiles of an MFMA
  const int tid = threadIdx.x, S = a.S, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, l32 = lane & 31;
  const int W0 = a.pol.width[0], W1 = TWO ? a.pol.width[1] : 0;
  const int W0p = (W0 + 31) & ~31, W1p = (W1 + 31) & ~31, WLp = TWO ? W1p : W0p;
  const MfLayout L = mf_layout(TWO, W0p, W1p, NR);
  float* const s_w0 = s_mem + L.w0; float* const s_b1 = s_mem + L.b1; float* const s_wl = s_mem + L.wl;
  float* const s_x = s_mem + L.x; float* const s_h = s_mem + L.h;
  {                                                                    // stage the small parts of the network
    for (int i = tid; i < W0p; i += MF_NT) {
      const bool in = i < W0;
      s_w0[4 * i + 0] = in ? a.pol.w[0][i * 3 + 0] : 0.0f; s_w0[4 * i + 1] = in ? a.pol.w[0][i * 3 + 1] : 0.0f;
      s_w0[4 * i + 2] = in ? a.pol.w[0][i * 3 + 2] : 0.0f; s_w0[4 * i + 3] = in ? a.pol.b[0][i] : 0.0f;
    }
    const int WL = TWO ? W1 : W0, ll = TWO ? 2 : 1;
    for (int i = tid; i < WLp + 4; i += MF_NT) s_wl[i] = i < WL ? a.pol.w[ll][i] : (i == WLp ? a.pol.b[ll][0] : 0.0f);
    if (TWO) for (int i = tid; i < W1p; i += MF_NT) s_b1[i] = i < W1 ? a.pol.b[1][i] : 0.0f;
    if constexpr (EXPLORE) {
      const float* const wls = a.ex.w_log_std;
      for (int i = tid; i < WLp + 4; i += MF_NT) s_mem[L.total + i] = (wls && i < WL) ? wls[i] : (i == WLp ? a.ex.b_log_std[0] : 0.0f);
    }
  }
  // ---- the rows: lane tid < NR owns row tid (whole envs) --------------------------------------------------------------------------------
  const int b0 = (int)blockIdx.x * a.epb;                              // the workgroup's first env
  const int n_env = min(a.epb, a.B - b0);
  const bool row = tid < NR;                                           // (waves 0 .. NR / 64 - 1: whole waves)
  const bool on = tid < n_env * S;
  const int el = on ? tid / S : 0, s = on ? tid - el * S : 0;
  const int b = b0 + el;
  const int64_t pair = (int64_t)b * S + s, total = (int64_t)a.B * S;
  PolShop sh;
  float x[3] = {0.0f, 0.0f, 0.0f};
  if (row) {
    sh.load(a, pair, b, s);
    sh.encode(sh.stock, sh.sales, sh.missed, x);                       // what the agent observes now: the policy's first input
    sh.orders_init();
    s_x[4 * tid + 0] = x[0]; s_x[4 * tid + 1] = x[1]; s_x[4 * tid + 2] = x[2];
  }
  // ---- layer 1's operands: this lane's weight rows (units mb * 32 + l32 of the wave's blocks mb = wave, wave + 4) ------------------------
  const int Q = W0p >> 2;                                              // k in fours
  const float* wrow[2]; bool wok[2], mact[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int mb = wave + 4 * m, u = mb * 32 + l32;
    mact[m] = TWO && mb * 32 < W1p;                                    // (wave-uniform)
    wok[m] = TWO && u < W1;
    wrow[m] = TWO ? a.pol.w[1] + (int64_t)(wok[m] ? u : 0) * W0 : nullptr;
  }
  auto ldw = [&](int q, int m) -> float4 {                             // W1[u][4q .. 4q + 3] of slot m, zero beyond the matrix
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (q < Q && mact[m]) {
      if (VEC) { if (wok[m] && 4 * q < W0) v = *(const float4*)(wrow[m] + 4 * q); }
      else if (wok[m]) {
        const int k = 4 * q;
        v.x = k < W0 ? wrow[m][k] : 0.0f; v.y = k + 1 < W0 ? wrow[m][k + 1] : 0.0f;
        v.z = k + 2 < W0 ? wrow[m][k + 2] : 0.0f; v.w = k + 3 < W0 ? wrow[m][k + 3] : 0.0f;
      }
    }
    return v;
  };
  // layer 0's share of this lane: row r0, units u0, u0 + UST, ...
  constexpr int UST = MF_NT / NR;
  const int r0 = tid & (NR - 1), u0 = tid / NR;
  __syncthreads();

  float* p_obs = a.io.obs + pair * 3; float* p_act = a.io.action_out + pair; float* p_rew = a.io.reward + pair;
  const bool has_ter = a.io.terminated != nullptr;                     // (uniform: a scalar branch)
  uint8_t* p_ter = a.io.terminated + pair; uint8_t* p_tru = a.io.truncated + pair;
  // EXPLORE: running pointers of the noise and the three planes; `nz` is the step's noise, loaded one step ahead
  const float* const s_ls = s_mem + L.total;
  const float* p_nz = nullptr; float *p_raw = nullptr, *p_lp = nullptr, *p_di = nullptr; float nz = 0.0f;
  if constexpr (EXPLORE) {
    p_nz = a.ex.noise + pair; p_raw = a.ex.raw_action + pair; p_lp = a.ex.logp + pair; p_di = a.ex.dist_inputs + pair * 2;
    if (on) nz = *p_nz;
  }
  for (int t = 0; t < a.T; ++t) {
    // ---- layer 0 (VALU): h0[u][r] = act(b + w.x0 + w.x1 + w.x2), k ascending ------------------------------------------------------------
    {
      const float4 xr = *(const float4*)(s_x + 4 * r0);
      for (int u = u0; u < W0p; u += UST) {
        const float4 w = *(const float4*)(s_w0 + 4 * u);
        float c = w.w;
        c = __fmaf_rn(w.x, xr.x, c); c = __fmaf_rn(w.y, xr.y, c); c = __fmaf_rn(w.z, xr.z, c);
        s_h[mf_hidx<NR>(u, r0)] = pol_act<ACT>(c);
      }
    }
    __syncthreads();
    if (TWO) {
      // ---- layer 1 (MFMA): acc[m][n] = units of block wave + 4m x rows of tile n; C = the bias, k-pairs ascending --------------------------
      mfma_f16 acc[2][NTILE];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        mfma_f16 c0;
#pragma unroll
        for (int r = 0; r < 16; ++r) c0[r] = mact[m] ? s_b1[(wave + 4 * m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl] : 0.0f;
#pragma unroll
        for (int n = 0; n < NTILE; ++n) acc[m][n] = c0;
      }
      // one trip: k = 4q .. 4q + 3 = two MFMA k-steps; this lane's half hl takes k = 4q + hl (step 2q) and 4q + 2 + hl (step 2q + 1)
      auto trip = [&](int q, const float4* v) __attribute__((always_inline)) {
        float be[NTILE], bo[NTILE];
#pragma unroll
        for (int n = 0; n < NTILE; ++n) {
          be[n] = s_h[mf_hidx<NR>(4 * q + hl, n * 32 + l32)];
          bo[n] = s_h[mf_hidx<NR>(4 * q + 2 + hl, n * 32 + l32)];
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          if (!mact[m]) continue;
          const float ae = hl ? v[m].y : v[m].x, ao = hl ? v[m].w : v[m].z;
#pragma unroll
          for (int n = 0; n < NTILE; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae, be[n], acc[m][n], 0, 0, 0);
#pragma unroll
          for (int n = 0; n < NTILE; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(ao, bo[n], acc[m][n], 0, 0, 0);
        }
      };
      float4 p0[2], p1[2], p2[2], p3[2];                               // the weights of trips q .. q + 3 in flight
#pragma unroll
      for (int m = 0; m < 2; ++m) { p0[m] = ldw(0, m); p1[m] = ldw(1, m); p2[m] = ldw(2, m); p3[m] = ldw(3, m); }
      for (int q = 0; q < Q; q += 4) {                                 // (Q is a multiple of 8)
        trip(q, p0);
#pragma unroll
        for (int m = 0; m < 2; ++m) p0[m] = ldw(q + 4, m);
        trip(q + 1, p1);
#pragma unroll
        for (int m = 0; m < 2; ++m) p1[m] = ldw(q + 5, m);
        trip(q + 2, p2);
#pragma unroll
        for (int m = 0; m < 2; ++m) p2[m] = ldw(q + 6, m);
        trip(q + 3, p3);
#pragma unroll
        for (int m = 0; m < 2; ++m) p3[m] = ldw(q + 7, m);
      }
      __syncthreads();                                                 // every wave has read h0: h1 replaces it in the image
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        if (!mact[m]) continue;
#pragma unroll
        for (int n = 0; n < NTILE; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            s_h[mf_hidx<NR>((wave + 4 * m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl, n * 32 + l32)] = pol_act<ACT>(acc[m][n][r]);
      }
      __syncthreads();
    }
    if (row) {
      // ---- the output layer (VALU): y = b + sum over k ascending of w[k] h[k][row] ---------------------------------------------------
      float y = s_wl[WLp];
      for (int k0 = 0; k0 < WLp; k0 += 4) {
        const float4 w = *(const float4*)(s_wl + k0);
        y = __fmaf_rn(w.x, s_h[mf_hidx<NR>(k0 + 0, tid)], y); y = __fmaf_rn(w.y, s_h[mf_hidx<NR>(k0 + 1, tid)], y);
        y = __fmaf_rn(w.z, s_h[mf_hidx<NR>(k0 + 2, tid)], y); y = __fmaf_rn(w.w, s_h[mf_hidx<NR>(k0 + 3, tid)], y);
      }
      PolDraw dr;
      if constexpr (EXPLORE) {                                         // the log-std output: the same walk over the image
        float ls = s_ls[WLp];
        for (int k0 = 0; k0 < WLp; k0 += 4) {
          const float4 w = *(const float4*)(s_ls + k0);
          ls = __fmaf_rn(w.x, s_h[mf_hidx<NR>(k0 + 0, tid)], ls); ls = __fmaf_rn(w.y, s_h[mf_hidx<NR>(k0 + 1, tid)], ls);
          ls = __fmaf_rn(w.z, s_h[mf_hidx<NR>(k0 + 2, tid)], ls); ls = __fmaf_rn(w.w, s_h[mf_hidx<NR>(k0 + 3, tid)], ls);
        }
        dr = pol_draw(a.pol, y, a.ex.w_log_std ? ls : s_ls[WLp], nz);      // (no row: ls = b_log_std[0])
      }
      const float action = EXPLORE ? dr.action : pol_action(a.pol, y);
      // ---- PhantomEnv.step for the pair ---------------------------------------------------------------------------------------------------
      const int D = sh.orders<EXO>(a, t, b, s);
      float ob[3], rw;
      const bool trunc = sh.advance(a, action, D, ob, rw);
      if (on) {                                                        // the trajectory row, rollout.py:361-389
        if constexpr (EXPLORE) {                                       // the next step's noise, issued ahead of this step's stores
          p_nz += total;
          if (t + 1 < a.T) nz = *p_nz;
        }
        p_obs[0] = ob[0]; p_obs[1] = ob[1]; p_obs[2] = ob[2];
        *p_act = action;
        *p_rew = rw;
        if (has_ter) { *p_ter = 0; p_ter += total; }
        *p_tru = trunc ? 1 : 0;
        p_obs += total * 3; p_act += total; p_rew += total; p_tru += total;
        if constexpr (EXPLORE) {
          *p_raw = dr.z; *p_lp = dr.logp; *(pol_f2u*)p_di = (pol_f2u){dr.y, dr.ls};
          p_raw += total; p_lp += total; p_di += total * 2;
        }
      }
      sh.next(trunc, ob, x);                                           // the caller's env.reset() at an episode's end; the next input
      s_x[4 * tid + 0] = x[0]; s_x[4 * tid + 1] = x[1]; s_x[4 * tid + 2] = x[2];
    }
    __syncthreads();                                                   // x is written, the image read
  }
  if (on) sh.store(a, pair, b, s, x);
}

template <int ACT, bool TWO, bool EXO, int NR, bool VEC>
__global__ __launch_bounds__(MF_NT) void phx_sc_rollout_policy_mfma_kernel(const PolArgs a) { pol_rollout_mfma<ACT, TWO, EXO, NR, VEC, false>(a); }

template <int ACT, bool TWO, bool EXO, int NR, bool VEC>
__global__ __launch_bounds__(MF_NT) void phx_sc_rollout_policy_mfma_explore_kernel(const PolArgsX a) { pol_rollout_mfma<ACT, TWO, EXO, NR, VEC, true>(a); }

hipError_t phx_launch_sc_rollout_policy_mfma(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st) {
  PolArgsX a; memset(&a, 0, sizeof a);
  a.B = sp.B; a.S = sp.S; a.T = io.T; a.num_steps = sp.num_steps; a.n_exo = sp.n_exo;
  a.seed = sp.seed; a.env_offset = sp.env_offset;
  a.stock = (int32_t*)sp.f[F_SHOP_STOCK]; a.sales = (int32_t*)sp.f[F_SHOP_SALES]; a.missed = (int32_t*)sp.f[F_SHOP_MISSED];
  a.delivered = (int32_t*)sp.f[F_SHOP_DELIVERED]; a.env_step = (int32_t*)sp.f[F_ENV_STEP]; a.env_tick = (int32_t*)sp.f[F_ENV_TICK];
  a.shop_norm = sp.shop_norm; a.shop_cust_ptr = sp.shop_cust_ptr; a.shop_cust_exo = sp.shop_cust_exo;
  a.io = io; a.pol = *io.policy;
  const bool explore = io.explore != nullptr;
  if (explore) a.ex = *io.explore;
  const bool two = a.pol.n_hidden == 2;
  const int NR = sp.S <= 64 ? 64 : 128;                                // (phx_sc_policy_unsupported: S <= 128)
  a.epb = NR / sp.S;
  const dim3 grid((unsigned)((sp.B + a.epb - 1) / a.epb));
  const int W0p = (a.pol.width[0] + 31) & ~31, W1p = two ? (a.pol.width[1] + 31) & ~31 : 0;
  const int WLp = two ? W1p : W0p;
  const size_t lds = ((size_t)mf_layout(two, W0p, W1p, NR).total + (explore ? WLp + 4 : 0)) * sizeof(float);      // <= 135 + 1 KB (NR = 128, 256 units)
  const bool vec = two && (a.pol.width[0] & 3) == 0 && ((uintptr_t)a.pol.w[1] & 15u) == 0;
  phx_note_kernel(explore ? "phx_sc_rollout_policy_mfma_explore_kernel" : "phx_sc_rollout_policy_mfma_kernel");
  const PolArgs& a0 = a;                                               // (the deterministic kernels take the base block)
  // (more than 64 KB of dynamic LDS needs the attribute: per device and instantiation, result checked)
#define MF_GO1(KERNEL_, ARGS_, EXO_, ACT_, TWO_, NR_, VEC_) do { \
    static PhxPerDeviceOnce attr_done; int dev = 0; (void)hipGetDevice(&dev); \
    if (!attr_done.done(dev)) { \
      const hipError_t ae = hipFuncSetAttribute((const void*)KERNEL_<ACT_, TWO_, EXO_, NR_, VEC_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      if (ae != hipSuccess) return ae; \
      attr_done.mark(dev); } \
    hipLaunchKernelGGL((KERNEL_<ACT_, TWO_, EXO_, NR_, VEC_>), grid, dim3(MF_NT), lds, st, ARGS_); } while (0)
#define MF_GO(EXO_, ACT_, TWO_, NR_, VEC_) do { \
    if (explore) MF_GO1(phx_sc_rollout_policy_mfma_explore_kernel, a, EXO_, ACT_, TWO_, NR_, VEC_); \
    else MF_GO1(phx_sc_rollout_policy_mfma_kernel, a0, EXO_, ACT_, TWO_, NR_, VEC_); } while (0)
#define MF_LAUNCH(ACT_, TWO_, NR_, VEC_) do { if (io.exo) MF_GO(true, ACT_, TWO_, NR_, VEC_); else MF_GO(false, ACT_, TWO_, NR_, VEC_); } while (0)
#define MF_NR(ACT_) do { \
    if (!two) { if (NR == 64) MF_LAUNCH(ACT_, false, 64, false); else MF_LAUNCH(ACT_, false, 128, false); } \
    else if (vec) { if (NR == 64) MF_LAUNCH(ACT_, true, 64, true); else MF_LAUNCH(ACT_, true, 128, true); } \
    else { if (NR == 64) MF_LAUNCH(ACT_, true, 64, false); else MF_LAUNCH(ACT_, true, 128, false); } } while (0)
  if (a.pol.activation == PHX_ACT_TANH) MF_NR(PHX_ACT_TANH);
  else if (a.pol.activation == PHX_ACT_HARD_TANH) MF_NR(PHX_ACT_HARD_TANH);
  else MF_NR(PHX_ACT_RELU);
#undef MF_NR
#undef MF_LAUNCH
#undef MF_GO
#undef MF_GO1
  return hipGetLastError();
}
