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
 * Validity planes are out of scope of phx_gae: FSM / Stackelberg envs, whose step dicts omit keys (obs_valid / reward_valid of
 * phx_rollout_io), have per-agent trajectories with holes.  phx_gae_masked below is the scan for those; phx_gae serves plain
 * envs, where it moves fewer bytes.
 *
 * phx_gae_masked.  A row t of column n is a trajectory row where acted[t][n] != 0 (the agent held an observation and acted at
 * step t).  The reference hands an agent its reward together with its NEXT observation, rows later, and a multi-agent sampler
 * credits an action with every reward that arrives until the agent's next observation.  So: the segment of trajectory row t0 is
 * the rows from t0 up to, and excluding, the column's next trajectory row; the segment's reward is the sum of its present
 * rewards (reward_valid == 1), added from the last one down; the first cut row of the segment closes it (rewards after that row
 * are dropped: they belong to no action), and that cut row's terminated flag and vf_next element decide the bootstrap value;
 * the advantage chain links trajectory rows only.  Every operation is the correctly rounded f32 one, gl = gamma * lambda.
 * A column is walked on its own, t from T - 1 down to 0, carrying acc, nv, adv_next, v_next (f32) and empty, cut, term (bool),
 * which start as acc = nv = adv_next = v_next = +0.0f, empty = true, cut = true, term = false:
 *
 *   te   = terminated != NULL && terminated[t][n] != 0
 *   crow = te || truncated[t][n] != 0 || t == T - 1
 *   if (crow) { empty = true; cut = true; term = te; nv = te ? +0.0f : vf_next[t][n]; }
 *   if (reward_valid[t][n] == 1) { acc = empty ? reward[t][n] : reward[t][n] + acc; empty = false; }
 *   if (acted[t][n] != 0) {
 *       rs  = empty ? +0.0f : acc;           v = vf_pred[t][n]
 *       nvv = term ? +0.0f : (cut ? nv : v_next);             c = cut ? +0.0f : adv_next
 *       d   = fmaf(gamma, nvv, rs) - v;      adv = fmaf(gl, c, d)
 *       advantage[t][n] = adv;  value_target[t][n] = adv + v;  reward_sum[t][n] = rs
 *       adv_next = adv; v_next = v; empty = true; cut = false; term = false
 *   } else advantage[t][n] = value_target[t][n] = reward_sum[t][n] = +0.0f
 *
 * Everything that enters arithmetic is selected, never multiplied by zero: vf_pred at non-trajectory rows, reward where
 * reward_valid != 1 and vf_next anywhere but the closing cut row of a segment may hold anything, NaN included (the planes
 * must still be readable).  Two properties (tests/test_gae_masked_cpu.py).  Compaction: for every column, the outputs at its
 * trajectory rows equal, bit for bit, phx_gae on the column compacted to those rows -- reward: the segment sums; vf_pred: the
 * trajectory rows' own; truncated = 1, with terminated and vf_next taken from the closing cut row, wherever a segment holds a
 * cut row or row T - 1.  Reduction: with acted == NULL && reward_valid == NULL the result equals phx_gae's bit for bit and
 * reward_sum equals reward, with -0.0 among the inputs too (the first present reward is assigned, not added to +0.0f).
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

typedef struct phx_gae_masked_io {
  int32_t T;  int32_t reserved0;        /* rows; 0                                              */
  int64_t N;                            /* columns per row                                      */
  float   gamma, lambda;                /* each in [0, 1]                                       */
  const float*   reward;                /* [T][N]; read where reward_valid == 1                 */
  const float*   vf_pred;               /* [T][N], read at trajectory rows, or NULL == +0.0f    */
  const float*   vf_next;               /* [T][N], read at the closing cut row of a segment unless it terminates, or NULL == +0.0f */
  const uint8_t* terminated;            /* [T][N] or NULL == all zero                           */
  const uint8_t* truncated;             /* [T][N]                                               */
  const uint8_t* acted;                 /* [T][N] or NULL == all one: != 0 <=> row t is a trajectory row of column n */
  const uint8_t* reward_valid;          /* [T][N] or NULL == all one: the rollout's plane; ONLY the value 1 counts (0 absent, 2 None) */
  float*   advantage;                   /* [T][N]; +0.0f at rows that are no trajectory rows    */
  float*   value_target;                /* [T][N] or NULL: not written                          */
  float*   reward_sum;                  /* [T][N] or NULL: not written; the segment's reward    */
} phx_gae_masked_io;                    /* 104 bytes */

/* Alignment, element offsets, overlap and return codes as phx_gae: reward, vf_pred and vf_next 4 bytes, the three outputs 16
 * bytes; PHX_EINVAL with a phx_last_error text (io or a required pointer -- reward, truncated, advantage -- NULL; a misaligned
 * pointer; T < 1 or N < 1; gamma or lambda outside [0, 1], NaN included; reserved0 != 0; N beyond one launch's grid), and
 * nothing is launched then.  All three output planes are written everywhere.  After a successful call phx_last_kernel() reads
 * "phx_gae_masked_kernel". */
int phx_gae_masked(const phx_gae_masked_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_GAE_H */
