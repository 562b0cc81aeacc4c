// phx_sc_policy.h -- what the two device-policy rollout kernels share (phx_sc_policy.hip: one lane per (env, shop) evaluates the MLP on
// VALU; phx_sc_policy_mfma.hip: a workgroup evaluates it for its rows with f32 MFMA): the launch arguments, the activations of
// phx_policy_mlp (include/phantom_amd.h) and the plain supply chain's (env, shop) row -- its state in registers, the observation it
// encodes, the customers' orders of a step and the closed form of the step itself.
#pragma once
#include "phx_launch.h"

struct PolArgs {
  int32_t B, S, epb, T, num_steps, n_exo;
  uint64_t seed; int64_t env_offset;
  int32_t *stock, *sales, *missed, *delivered, *env_step, *env_tick;
  const int32_t* shop_norm; const int32_t* shop_cust_ptr; const int32_t* shop_cust_exo;
  phx_rollout_io io;
  phx_policy_mlp pol;
};
// the exploring kernels' arguments: the same block and the io's phx_policy_explore (a host struct) copied in by value
struct PolArgsX : PolArgs {
  phx_policy_explore ex;
};

// PHX_ACT_TANH as the header defines it, step for step: every operation is a correctly rounded f32 one (__fmaf_rn, __fmul_rn, __fdiv_rn),
// so the value is the definition's on every machine
__device__ __forceinline__ float pol_tanh(float c) {
  const float a = __builtin_fabsf(c);
  float t;
  if (!(a < PHX_TANH_SAT)) t = 1.0f;
  else if (a < PHX_TANH_SMALL) t = a;
  else {
    const float s = __fmul_rn(a, a);
    float p = PHX_TANH_A13;
    p = __fmaf_rn(p, s, PHX_TANH_A11); p = __fmaf_rn(p, s, PHX_TANH_A9); p = __fmaf_rn(p, s, PHX_TANH_A7);
    p = __fmaf_rn(p, s, PHX_TANH_A5); p = __fmaf_rn(p, s, PHX_TANH_A3); p = __fmaf_rn(p, s, PHX_TANH_A1);
    float q = PHX_TANH_B6;
    q = __fmaf_rn(q, s, PHX_TANH_B4); q = __fmaf_rn(q, s, PHX_TANH_B2); q = __fmaf_rn(q, s, PHX_TANH_B0);
    t = __fdiv_rn(__fmul_rn(a, p), q);
    t = t > 1.0f ? 1.0f : t;
  }
  return __builtin_copysignf(t, c);
}

// act(c).  ReLU and hard-tanh as ONE v_med3_f32: ReLU = the median of (c, 0, +inf), hard-tanh = the median of (c, -1, 1).  Finite c: the
// values of the header's definition (c > 0 ? c : +0 / the two-sided clip); a -0 that med3 may let through where the definition says +0
// changes no sum's value and the definition's closing "+ 0.0f" removes it from the action.
template <int ACT>
__device__ __forceinline__ float pol_act(float c) {
  if (ACT == PHX_ACT_TANH) return pol_tanh(c);
  if (ACT == PHX_ACT_HARD_TANH) return __builtin_amdgcn_fmed3f(c, -1.0f, 1.0f);
  return __builtin_amdgcn_fmed3f(c, 0.0f, __builtin_inff());
}

// the action from the network's output y: a = fmaf(out_scale, y, out_bias), clipped; (+ 0.0f: an exact zero leaves as +0)
__device__ __forceinline__ float pol_action(const phx_policy_mlp& p, float y) {
  const float av = __fmaf_rn(p.out_scale, y, p.out_bias);
  return (av < p.out_lo ? p.out_lo : (av > p.out_hi ? p.out_hi : av)) + 0.0f;
}

// Gaussian exploration (include/phantom_amd.h, phx_policy_explore), step for step with correctly rounded f32 operations, like pol_tanh.
// exp(l) for a clamped log-std |l| <= 20: Cody-Waite reduction by ln 2, a degree-7 Taylor polynomial, ldexp (exact for |n| <= 29)
__device__ __forceinline__ float pol_exp(float l) {
  const float n = __builtin_rintf(__fmul_rn(l, PHX_EXP_LOG2E));        // (v_rndne_f32: half to even)
  float r = __fmaf_rn(-n, PHX_EXP_LN2_HI, l);
  r = __fmaf_rn(-n, PHX_EXP_LN2_LO, r);
  float p = PHX_EXP_C7;
  p = __fmaf_rn(p, r, PHX_EXP_C6); p = __fmaf_rn(p, r, PHX_EXP_C5); p = __fmaf_rn(p, r, PHX_EXP_C4); p = __fmaf_rn(p, r, PHX_EXP_C3);
  p = __fmaf_rn(p, r, PHX_EXP_C2); p = __fmaf_rn(p, r, PHX_EXP_C1); p = __fmaf_rn(p, r, PHX_EXP_C0);
  return __builtin_ldexpf(p, (int)n);
}

// the Gaussian log-density of z = fmaf(std, noise, y), stated through the noise: -noise^2 / 2 - l - ln(2 pi) / 2
__device__ __forceinline__ float pol_logp(float noise, float l) {
  return __fmaf_rn(-0.5f, __fmul_rn(noise, noise), __fsub_rn(-l, PHX_HALF_LN_2PI));
}

// the draw: (y, ls) as the header takes them (+ 0.0f), the clamped log-std, z, the env's action and log-density
struct PolDraw { float y, ls, z, logp, action; };
__device__ __forceinline__ PolDraw pol_draw(const phx_policy_mlp& p, float y, float ls, float noise) {
  PolDraw d;
  d.y = y + 0.0f; d.ls = ls + 0.0f;
  const float l = d.ls < PHX_LOG_STD_MIN ? PHX_LOG_STD_MIN : (d.ls > PHX_LOG_STD_MAX ? PHX_LOG_STD_MAX : d.ls);
  d.z = __fmaf_rn(pol_exp(l), noise, d.y);
  d.logp = pol_logp(noise, l);
  d.action = pol_action(p, d.z);
  return d;
}

// dist_inputs' (y, ls): one 8-byte store at a 4-byte aligned address (phx_policy_explore asks for 4 bytes)
typedef float pol_f2u __attribute__((ext_vector_type(2), aligned(4)));

// One (env, shop) row of a plain supply-chain env: its state lives in registers for the launch.
struct PolShop {
  int stock, sales, missed, delivered, step; uint32_t tick;
  int norm_i; float norm_f; int c0, K; int64_t genv;
  float r_stock, r_norm; bool norm_small;
  bool small_k; uint32_t pK; float inv_pK;
  RngQuadCache quad;

  // the state and the shop's constants (every lane of the wave calls it: `orders_init` below is a wave vote)
  __device__ __forceinline__ void load(const PolArgs& a, int64_t pair, int b, int s) {
    stock = a.stock[pair]; sales = a.sales[pair]; missed = a.missed[pair]; delivered = a.delivered[pair];
    step = a.env_step[b]; tick = (uint32_t)a.env_tick[b];
    // (a "use" of every loaded word HERE: `delivered` is overwritten by the first step without ever being read, and the s_waitcnt vmcnt(0) that
    //  protects its register from the load still in flight would otherwise sit inside the step loop -- where it waits for the row's stores)
    asm volatile("" :: "v"(stock), "v"(sales), "v"(missed), "v"(delivered), "v"(step), "v"(tick));
    norm_i = a.shop_norm[s];
    norm_f = (float)norm_i;
    c0 = a.shop_cust_ptr[s]; K = a.shop_cust_ptr[s + 1] - c0;
    genv = a.env_offset + b;
    // the divisors never change: their reciprocals once (IEEE divisions), a quotient = a multiply and Markstein's correction (phx_dev.h: div_by_recip)
    r_stock = 1.0f / (float)PHX_SHOP_MAX_STOCK; r_norm = 1.0f / norm_f;
    norm_small = norm_i >= 1 && norm_i <= DIV_RECIP_N;
  }
  __device__ __forceinline__ void orders_init() {
    small_k = __all(K <= 6) != 0;
    pK = K <= 0 ? 1u : K == 1 ? 5u : K == 2 ? 25u : K == 3 ? 125u : K == 4 ? 625u : K == 5 ? 3125u : 15625u;
    inv_pK = K <= 0 ? 1.0f : K == 1 ? 0.2f : K == 2 ? 0.04f : K == 3 ? 0.008f : K == 4 ? 0.0016f : K == 5 ? 0.00032f : 0.000064f;
    quad.q = 0xffffffffu; quad.w[0] = quad.w[1] = quad.w[2] = quad.w[3] = 0u;
  }

  __device__ __forceinline__ void encode(int st, int sl, int ms, float* o) const {      // ShopAgent.encode_observation, supply_chain.py:124-134
    if (__builtin_expect(norm_small && (unsigned)(st | sl | ms) < (unsigned)DIV_RECIP_X, 1)) {
      o[0] = div_by_recip((float)st, (float)PHX_SHOP_MAX_STOCK, r_stock);
      o[1] = div_by_recip((float)sl, norm_f, r_norm);
      o[2] = div_by_recip((float)ms, norm_f, r_norm);
    } else if ((((unsigned)st + (1u << 24)) | ((unsigned)sl + (1u << 24)) | ((unsigned)ms + (1u << 24)) | ((unsigned)norm_i + (1u << 24))) < (2u << 24))
      shop_obs_f32(st, sl, ms, norm_f, o);
    else shop_obs(st, sl, ms, norm_i, o);
  }

  // the shop's customers' order sizes of step t summed, supply_chain.py:61-67: replayed from io.exo, or the device Philox stream (one
  // block serves four ticks)
  template <bool EXO>
  __device__ __forceinline__ int orders(const PolArgs& a, int t, int b, int s) {
    int D = 0;
    if (EXO) {
      const uint8_t* row = a.io.exo + ((int64_t)t * a.B + b) * a.n_exo;
      for (int k = 0; k < K; ++k) D += (int)row[a.shop_cust_exo[c0 + k]];
    } else {
      rng_quad_block(quad, a.seed, genv, tick, s);
      if (small_k) {                                                   // (uniform) every shop of the wave has at most six customers: one word, its first K base-5 digits
        uint32_t y, jr;
        if (__builtin_expect(!rng_split(rng_pick(quad.w, tick), y, jr), 0)) y = rng_group_y(a.seed, genv, tick, s, 0, 1);      // probability 3.3e-6
        y -= __umul24((uint32_t)((float)y * inv_pK), pK);              // y mod 5^K (exact through f32: tests/test_host_logic.py)
        D = rng_digit_sum6(y);
      } else D = rng_orders_from_block(quad.w, a.seed, genv, tick, s, K, nullptr, nullptr);
    }
    return D;
  }

  // PhantomEnv.step for the pair (env.py:239-303 with the supply chain's closed form): the new state, its observation `ob` and the
  // reward; true at the episode's last step
  __device__ __forceinline__ bool advance(const PolArgs& a, float action, int D, float* ob, float& rw) {
    const int req = dev_round_half_even(action), room = PHX_SHOP_MAX_STOCK - stock;      // decode_action :136-142 (the stock BEFORE the step)
    const int deliv = req < room ? req : room;
    const int sell = stock < D ? stock : D;                            // handle_order_request, order after order: sells what is left (:105-122)
    sales = sell; missed = D - sell;
    stock = stock - sell + deliv;                                      // handle_stock_response (:98-103): deliv <= 100 - stock
    delivered = deliv;
    const int t_ep = step + 1;
    const bool trunc = t_ep == a.num_steps;                            // truncations["__all__"], env.py:312-318
    encode(stock, sales, missed, ob);
    rw = (float)shop_reward(sales, stock);                             // compute_reward :147, rounded once to f32
    return trunc;
  }

  // after the trajectory row: the caller's env.reset() at an episode's end (ShopAgent.reset zeroes the stock, :149-150; sales stay,
  // App. B), and the policy's next input x
  __device__ __forceinline__ void next(bool trunc, const float* ob, float* x) {
    ++tick;
    if (trunc) {
      stock = 0; step = 0;
      encode(0, sales, missed, x);
    } else { step = step + 1; x[0] = ob[0]; x[1] = ob[1]; x[2] = ob[2]; }
  }

  __device__ __forceinline__ void store(const PolArgs& a, int64_t pair, int b, int s, const float* x) const {
    a.stock[pair] = stock; a.sales[pair] = sales; a.missed[pair] = missed; a.delivered[pair] = delivered;
    if (a.io.last_obs) { float* lo = a.io.last_obs + pair * 3; lo[0] = x[0]; lo[1] = x[1]; lo[2] = x[2]; }
    if (s == 0) { a.env_step[b] = step; a.env_tick[b] = (int32_t)tick; }
  }
};
