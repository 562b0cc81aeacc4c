/*
 * phantom_amd_traj.h -- the per-agent view of a rollout fragment whose trajectories have holes: for every row where an agent
 * acted, the observation it holds when its transition ends and the done flags of that transition, in one call.
 *
 * A fourth, additive header of libphantom_amd.so: nothing in phantom_amd.h, phantom_amd_gae.h or phantom_amd_vtrace.h changes
 * (PHX_ABI_VERSION stays 10, the return codes and phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).
 * Like phx_gae_masked the function takes no env handle: planes in, planes out, on the current device, asynchronously on `stream`.
 *
 * On FSM and Stackelberg envs the step dicts omit keys: an agent acts in some steps only (`acted`), and receives an observation
 * from some steps only (`new_obs_valid`, the rollout's obs_valid plane).  A column is one (env instance, strategic agent) pair of
 * a phx_rollout fragment, N = B * S, row t is step t.  The step-aligned planes new_obs[t] / terminated[t] / truncated[t] say what
 * step t returned; a learner that reads transitions (obs, action, reward, next obs, done) of ONE agent needs, at a row where the
 * agent acted, what the agent saw NEXT and whether its episode ended before it acted again.  phx_gae_masked's reward_sum is the
 * reward of that transition; this call gives the other three columns, over the same segments.
 *
 * Segments (exactly phx_gae_masked's).  A trajectory row of a column is a row t0 with acted[t0][n] != 0 (acted == NULL: every
 * row).  Its segment runs from t0 up to, and excluding, the column's next trajectory row t1 (none: t1 = T).  The segment's
 * CLOSING row is the first row in [t0, t1) with terminated != 0 or truncated != 0, or row T - 1 if it lies in the segment and no
 * such row precedes it.  last = the closing row if there is one, else t1 - 1.
 *
 * At a trajectory row t0:
 *
 *   next_row[t0][n]        = the greatest u in [t0, last] with new_obs_valid[u][n] != 0 (new_obs_valid == NULL: last), else -1:
 *                            the row whose new_obs the agent holds when the segment ends; -1: it still holds obs[t0]
 *   next_terminated[t0][n] = 1 if the closing row exists and terminated[close][n] != 0, else 0
 *   next_truncated[t0][n]  = 1 if the closing row exists, terminated[close][n] == 0 and truncated[close][n] != 0, else 0
 *                            (row T - 1 without a flag closes the scan and sets neither: the fragment's end is no episode's end)
 *   next_obs[t0][n][:]     = new_obs[next_row][n][:] if next_row >= 0, else obs[t0][n][:]      (D 32-bit words, COPIED: bit patterns
 *                            survive, NaN payloads and -0.0 included)
 *
 * At every other row next_row = -1, both flags are 0 and next_obs is +0.0f: every output plane is written everywhere.
 *
 * As a reverse scan per column, state nr = -1, term = false, trunc = false; for t from T - 1 down to 0:
 *
 *   c     = terminated[t][n] != 0 || truncated[t][n] != 0 || t == T - 1;      here = new_obs_valid[t][n] != 0 ? t : -1
 *   nr    = c ? here : (nr < 0 ? here : nr)
 *   term  = c ? terminated[t][n] != 0 : term;      trunc = c ? (terminated[t][n] == 0 && truncated[t][n] != 0) : trunc
 *   acted[t][n] != 0 ?  emit (nr, term, trunc), then nr = -1, term = trunc = false
 *                    :  emit (-1, 0, 0)
 *
 * (a) Reduction.  With acted == NULL and new_obs_valid == NULL every row is its own segment and its own closing-or-last row:
 * next_row[t] == t, next_terminated == (terminated != 0), next_truncated == (terminated == 0 && truncated != 0), and next_obs
 * equals new_obs bit for bit.
 *
 * (b) Unread elements.  Of obs and new_obs only the ONE selected source element of a trajectory row enters a result -- the words
 * are selected, never computed with -- so every other element may hold anything; the planes must be readable all the same (the
 * call may load any of their T * N * D words).
 *
 * (c) Completeness.  A trajectory row is a complete transition iff one of its two flags is set or next_row >= 0.  Only a
 * column's LAST trajectory row of the fragment can be incomplete (its answer lies in the next fragment).
 * (tests/traj_next_ref.py, tests/test_traj_next_cpu.py, tests/test_gpu_traj_next.py)
 */
#ifndef PHANTOM_AMD_TRAJ_H
#define PHANTOM_AMD_TRAJ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_traj_next_io {
  int32_t T;  int32_t D;                /* rows; f32 words per observation (used only when next_obs != NULL, then 1 <= D <= 64) */
  int64_t N;                            /* columns per row (B * S of a trajectory plane)        */
  const uint8_t* truncated;             /* [T][N]    required                                   */
  const uint8_t* terminated;            /* [T][N]    or NULL == all zero                        */
  const uint8_t* acted;                 /* [T][N]    or NULL == all one  (!= 0: a trajectory row, as in phx_gae_masked) */
  const uint8_t* new_obs_valid;         /* [T][N]    or NULL == all one  (the rollout's obs_valid plane; != 0 counts)   */
  const float*   obs;                   /* [T][N][D] what the agent acted on; required iff next_obs != NULL             */
  const float*   new_obs;               /* [T][N][D] what step t returned;    required iff next_obs != NULL             */
  int32_t* next_row;                    /* [T][N]    required                                   */
  uint8_t* next_terminated;             /* [T][N]    required                                   */
  uint8_t* next_truncated;              /* [T][N]    required                                   */
  float*   next_obs;                    /* [T][N][D] or NULL: no gather                         */
} phx_traj_next_io;                     /* 96 bytes */

/* Alignment: the inputs their natural one -- obs and new_obs 4 bytes, the flag planes none: rows [t0, t1) of a longer recording
 * are fine -- the four outputs 16 bytes.  Element offsets are 64-bit: T * N * D may exceed 2^31.  The outputs must not overlap
 * the inputs.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_traj_next: io, truncated, next_row, next_terminated or
 * next_truncated NULL; next_obs given without both obs and new_obs; D outside [1, 64] when next_obs is given; T < 1 or N < 1;
 * N beyond one launch's grid (N > 64 * (2^31 - 1), or with next_obs N * D > 256 * (2^31 - 1)); a misaligned pointer.  Nothing is
 * launched then.  PHX_EHIP: a launch failed.  After a successful call phx_last_kernel() reads "phx_traj_next_kernel" without
 * next_obs and "phx_traj_next_kernel+phx_traj_gather_kernel" with it (the gather is a second launch on the same stream). */
int phx_traj_next(const phx_traj_next_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_TRAJ_H */
