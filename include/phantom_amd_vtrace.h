/*
 * phantom_amd_vtrace.h -- V-trace value targets and policy-gradient advantages of rollout fragments, one launch.
 *
 * A third, additive header of libphantom_amd.so: nothing in phantom_amd.h or phantom_amd_gae.h changes (PHX_ABI_VERSION stays
 * 10, the return codes and phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like phx_gae the function
 * takes no env handle: planes in, planes out, on the current device, asynchronously on `stream`.
 *
 * It is the off-policy reverse scan of IMPALA and APPO (Espeholt et al. 2018, "IMPALA: Scalable Distributed Deep-RL with
 * Importance Weighted Actor-Learner Architectures"; RLlib's vtrace_torch.from_importance_weights) for every column of a
 * time-major trajectory plane at once.  A column is one (env instance, strategic agent) pair of a phx_rollout fragment:
 * N = B * S, row t is step t.  The value predictions and the two log-densities are inputs: behaviour_logp is what an exploring
 * rollout recorded (phx_policy_explore.logp), target_logp and the values are the learner's forward passes (batched GEMMs, which
 * torch does well); the scan over time, T dependent rounds of element-wise work, is what this call fuses.
 *
 * Definition.  Every operation is the correctly rounded f32 one (fmaf: one rounding; the library is built with
 * -ffp-contract=off), so the result is defined bit for bit.  Per element, independent of the scan:
 *
 *   lr  = target_logp[t][n] - behaviour_logp[t][n]
 *   l   = lr < -20.0f ? -20.0f : (lr > 20.0f ? 20.0f : lr)
 *   rho = exp(l)       exactly the PHX_EXP_* procedure of phantom_amd.h: n = rint(l * PHX_EXP_LOG2E) (half to even);
 *                      r = fmaf(-n, PHX_EXP_LN2_HI, l);  r = fmaf(-n, PHX_EXP_LN2_LO, r);  p = PHX_EXP_C7;
 *                      p = fmaf(p, r, PHX_EXP_C6); ... p = fmaf(p, r, PHX_EXP_C0);  rho = ldexp(p, n)  (exact: |n| <= 29;
 *                      within 0.92 ulp of exp over [-20, 20]; exp(+-0) == 1.0f exactly)
 *   rc  = rho < rho_bar ? rho : rho_bar
 *   cs  = lambda * (rho < c_bar ? rho : c_bar)         one multiply
 *   gc  = gamma * cs                                   one multiply
 *   rp  = rho < pg_rho_bar ? rho : pg_rho_bar
 *
 * Per column, t from T - 1 down to 0, carrying acc[t + 1], vs[t + 1] and vf_pred[t + 1]:
 *
 *   term = terminated != NULL && terminated[t][n] != 0
 *   cut  = term || truncated[t][n] != 0 || t == T - 1
 *   v    = vf_pred[t][n]
 *   nv   = term ? +0.0f : (cut ? vf_next[t][n] : vf_pred[t + 1][n])
 *   nvs  = term ? +0.0f : (cut ? vf_next[t][n] : vs[t + 1][n])
 *   c    = cut  ? +0.0f : acc[t + 1]
 *   td   = fmaf(gamma, nv, reward[t][n]) - v
 *   acc  = fmaf(gc, c, rc * td)                        (rc * td rounded, then one fmaf)
 *   vs[t][n]           = acc + v
 *   pg_advantage[t][n] = rp * (fmaf(gamma, nvs, reward[t][n]) - v)
 *
 * nv, nvs and c are selected, never multiplied by zero: what the unread elements of vf_next hold does not matter, NaN included
 * -- but the plane must be readable (the kernel may load any of its T * N elements).  A NULL vf_next reads as +0.0f everywhere.
 * Every input the definition reads must be finite.
 *
 * (a) Relation to RLlib.  With no flag set the only cut is row T - 1, and vf_next[T - 1] is from_importance_weights'
 * bootstrap_value: the result is then from_importance_weights(log_rhos = target_logp - behaviour_logp, discounts = gamma,
 * rewards, values = vf_pred, bootstrap_value, clip_rho_threshold = rho_bar, clip_pg_rho_threshold = pg_rho_bar) with its
 * cs = lambda * min(c_bar, rho) (RLlib: c_bar = 1, lambda = 1).  A terminated row is RLlib's discount = 0 at that row.  A
 * truncated row INSIDE the fragment cuts both traces and bootstraps from V(new_obs), as phx_gae does: episodes of this library's
 * envs end by truncation and reset inside a fragment, and the row after the cut belongs to another episode.
 *
 * (b) The clamp to +-20 is the domain of the defined exp.  It changes rc, cs and rp only where a threshold exceeds e^20
 * (4.85e8), or where rho < e^-20: an importance factor below 2.1e-9 is replaced by 2.1e-9.
 *
 * (c) Reduction.  With target_logp equal to behaviour_logp element for element (the same pointer is allowed) and all three
 * thresholds >= 1: lr = +-0, rho == 1.0f exactly, rc = 1, gc = gamma * lambda, and vs equals phx_gae's value_target bit for bit
 * for the same gamma, lambda and planes (acc is phx_gae's advantage); pg_advantage is then the one-step
 * fmaf(gamma, nvs, reward) - v.  (tests/test_vtrace_cpu.py, tests/test_gpu_vtrace.py)
 */
#ifndef PHANTOM_AMD_VTRACE_H
#define PHANTOM_AMD_VTRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_vtrace_io {
  int32_t T;  int32_t reserved0;        /* rows; 0                                              */
  int64_t N;                            /* columns per row (B * S of a trajectory plane)        */
  float   gamma, lambda;                /* each in [0, 1]                                       */
  float   rho_bar, c_bar, pg_rho_bar;   /* clip thresholds, each finite and > 0 (RLlib: clip_rho_threshold, 1.0, clip_pg_rho_threshold) */
  float   reserved1;                    /* 0                                                    */
  const float*   reward;                /* [T][N]                                               */
  const float*   vf_pred;               /* [T][N] V(obs the policy acted on): required          */
  const float*   vf_next;               /* [T][N] V(new_obs[t]); READ ONLY at cut rows that are not terminated; NULL == +0.0f */
  const float*   behaviour_logp;        /* [T][N] log mu(a|x): the rollout's action_logp        */
  const float*   target_logp;           /* [T][N] log pi(a|x) under the learner's weights       */
  const uint8_t* terminated;            /* [T][N] or NULL == all zero                           */
  const uint8_t* truncated;             /* [T][N]                                               */
  float*   vs;                          /* [T][N] the V-trace value targets                     */
  float*   pg_advantage;                /* [T][N] or NULL: not written                          */
} phx_vtrace_io;                        /* 112 bytes */

/* Alignment: the five f32 inputs 4 bytes (rows [t0, t1) of a longer recording are fine), the two outputs 16 bytes.  Element
 * offsets are 64-bit: T * N may exceed 2^31.  The outputs must not overlap the inputs.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_vtrace: io or a required pointer (every pointer but
 * vf_next, terminated and pg_advantage) NULL; a misaligned pointer; T < 1 or N < 1; N beyond one launch's grid; gamma or lambda
 * outside [0, 1] (NaN included); a threshold that is not finite or not > 0; reserved0 or reserved1 nonzero.  Nothing is launched
 * then.  PHX_EHIP: the launch failed.  After a successful call phx_last_kernel() reads "phx_vtrace_kernel". */
int phx_vtrace(const phx_vtrace_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_VTRACE_H */
