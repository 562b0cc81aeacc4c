/*
 * phantom_amd_gae.h -- advantages and value targets of rollout fragments (generalised advantage estimation), one launch.
 *
 * A second, additive header of libphantom_amd.so: nothing in phantom_amd.h changes (PHX_ABI_VERSION stays 10, the return
 * codes and phx_last_error / phx_last_kernel are the ones declared there).  The function takes no env handle: like
 * phx_pack_flags it works on planes, on the current device, asynchronously on `stream`.
 *
 * It is RLlib's compute_advantages(use_gae=True) (ray/rllib/evaluation/postprocessing.py) for every column of a
 * time-major trajectory plane at once: per agent trajectory, with last_r = 0 where the trajectory terminated and
 * last_r = V(last new_obs) where it was truncated or the fragment ends.  A column is one (env instance, strategic agent)
 * pair of a phx_rollout fragment: N = B * S, row t is step t.  The value predictions are inputs: the critic is the
 * caller's (a batched GEMM over T * N rows, which torch does well); the reverse scan over time is what this call fuses.
 *
 * Definition.  Every operation is the correctly rounded f32 one (fmaf: one rounding), so the result is defined bit for
 * bit.  With gl = gamma * lambda (one f32 multiply), each column n is walked on its own, t from T - 1 down to 0:
 *
 *   term = terminated != NULL && terminated[t][n] != 0
 *   cut  = term || truncated[t][n] != 0 || t == T - 1
 *   nv   = term ? +0.0f : (cut ? vf_next[t][n] : vf_pred[t + 1][n])
 *   c    = cut  ? +0.0f : advantage[t + 1][n]
 *   d    = fmaf(gamma, nv, reward[t][n]) - vf_pred[t][n]
 *   advantage[t][n]    = fmaf(gl, c, d)
 *   value_target[t][n] = advantage[t][n] + vf_pred[t][n]
 *
 * A NULL vf_pred / vf_next reads as +0.0f everywhere; with vf_pred == NULL and lambda = 1 the advantages are the
 * discounted returns of compute_advantages(use_critic=False).  Inputs must be finite (nv and c are selected, never
 * multiplied by zero, so what the unread elements of vf_next hold does not matter -- but the plane must be readable:
 * the kernel may load any of its T * N elements).
 *
 * Out of scope: validity planes.  FSM / Stackelberg envs, whose step dicts omit keys (obs_valid / reward_valid of
 * phx_rollout_io), have per-agent trajectories with holes; this call serves plain envs, as PhantomEnv.sample() does.
 */
#ifndef PHANTOM_AMD_GAE_H
#define PHANTOM_AMD_GAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_gae_io {
  int32_t T;  int32_t reserved0;        /* rows; 0                                              */
  int64_t N;                            /* columns per row (B * S of a trajectory plane)        */
  float   gamma, lambda;                /* each in [0, 1]                                       */
  const float*   reward;                /* [T][N]                                               */
  const float*   vf_pred;               /* [T][N] V(obs the policy acted on), or NULL == +0.0f  */
  const float*   vf_next;               /* [T][N] V(new_obs[t]); READ ONLY at cut rows that are not terminated; NULL == +0.0f */
  const uint8_t* terminated;            /* [T][N] or NULL == all zero                           */
  const uint8_t* truncated;             /* [T][N]                                               */
  float*   advantage;                   /* [T][N]                                               */
  float*   value_target;                /* [T][N] or NULL: not written                          */
} phx_gae_io;

/* Alignment: reward, vf_pred and vf_next 4 bytes (rows [t0, t1) of a longer recording are fine), the two outputs 16 bytes.
 * Element offsets are 64-bit: T * N may exceed 2^31.  The outputs must not overlap the inputs.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text: io or a required pointer (reward, truncated, advantage) NULL;
 * a misaligned pointer; T < 1 or N < 1; gamma or lambda outside [0, 1] (NaN included); reserved0 != 0.  Nothing is launched
 * then.  PHX_EHIP: the launch failed.  After a successful call phx_last_kernel() reads "phx_gae_kernel". */
int phx_gae(const phx_gae_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_GAE_H */
