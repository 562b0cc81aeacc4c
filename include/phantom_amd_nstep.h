/*
 * phantom_amd_nstep.h -- n-step transitions of a rollout fragment for replay learners (DQN / SAC / TD3 / DDPG with n_step > 1):
 * for every row where an agent acted, the discounted sum of the next n rewards of ITS OWN transitions, the observation n of its
 * transitions later, the done flags of the last transition folded and the discount to bootstrap with, in one call.
 *
 * A sixth, additive header of libphantom_amd.so: nothing in phantom_amd.h, phantom_amd_gae.h, phantom_amd_vtrace.h,
 * phantom_amd_traj.h or phantom_amd_compact.h changes (PHX_ABI_VERSION stays 10, the return codes and phx_last_error /
 * phx_last_kernel are the ones declared in phantom_amd.h).  Like the other five the function takes no env handle: planes in, planes
 * out, on the current device, asynchronously on `stream`.
 *
 * A column is one (env instance, strategic agent) pair of a phx_rollout fragment, N = B * S, row t is step t.  The inputs describe
 * TRANSITIONS, one per trajectory row (a row with acted != 0; acted == NULL: every row): on an FSM / Stackelberg env `reward` is
 * phx_gae_masked's reward_sum and truncated / terminated / next_row / next_obs are phx_traj_next's four outputs; on a plain env
 * they are the step-aligned planes of the rollout itself (next_row == NULL, next_obs = the observations plane).  The next
 * transition of an agent lies a data-dependent number of rows later, a chain stops at the agent's own done flags, and the last
 * trajectory row of a column may be an incomplete transition (phantom_amd_traj.h (c)).
 *
 * Every operation is the correctly rounded f32 one.  Per column n, for every row t:
 *
 *   succ_row[t][n] = the smallest t' > t with acted[t'][n] != 0, else -1.  It is written at EVERY row, trajectory row or not.  With
 *                    acted == NULL it is not written (nor read): the successor of t is t + 1 for t < T - 1, else none.
 *
 * For a trajectory row u of the column:
 *
 *   term(u)     = terminated != NULL && terminated[u][n] != 0
 *   trunc(u)    = !term(u) && truncated[u][n] != 0
 *   complete(u) = term(u) || trunc(u) || next_row == NULL || next_row[u][n] >= 0
 *
 * At a trajectory row t0, start with u = t0, m = 0, p = 1.0f:
 *
 *   loop:  cmp = complete(u)
 *          if (m > 0 && !cmp) break                       an incomplete transition is never folded into an earlier row
 *          G = (m == 0) ? reward[u][n] : fmaf(p, reward[u][n], G)      the first reward is ASSIGNED: -0.0 survives, n = 1 is the identity
 *          last = u;  m += 1;  p = p * gamma              one f32 multiply: p is gamma^m by repeated multiplication
 *          if (!cmp || term(u) || trunc(u) || m == n) break
 *          u = the successor of u;  if (none) break
 *   nstep_reward[t0][n]     = G;      nstep_discount[t0][n] = p;      nstep_last[t0][n] = last
 *   nstep_terminated[t0][n] = term(last);      nstep_truncated[t0][n] = trunc(last)
 *   nstep_next_row[t0][n]   = next_row == NULL ? last : next_row[last][n]
 *   nstep_next_obs[t0][n][:] = next_obs[last][n][:]       (D 32-bit words, COPIED as integers: NaN payloads and -0.0 survive)
 *
 * At every other row the outputs are +0.0f, +0.0f, -1, 0, 0, -1 and D words +0.0f: every output plane is written everywhere.
 * A learner's target is  nstep_reward + nstep_discount * (1 - nstep_terminated) * Q(nstep_next_obs).
 *
 * (a) Reduction.  With n = 1 the outputs at trajectory rows are the inputs bit for bit: nstep_reward == reward, nstep_last == t0,
 * nstep_discount == (float)gamma (1.0f * gamma), the flags normalised as above (0 / 1, terminated wins), nstep_next_row == next_row
 * (t0 without it) and nstep_next_obs == next_obs.
 *
 * (b) Relation to RLlib.  On one plain episode without holes (acted == NULL, next_row == NULL, the only flag in the episode's last
 * row) this is adjust_nstep: at row t it folds m = min(n, rows left) rewards, sum over k < m of gamma^k reward[t + k], takes new_obs
 * and the done flags of row t + m - 1, and makes the discount gamma^m explicit, which adjust_nstep leaves to the learner as
 * gamma ** n_step whatever m is (adjust_nstep adds in place in the batch's dtype; here the sum is the fmaf chain above).
 *
 * (c) Unread elements.  `reward` at rows that are no trajectory rows, `reward` at an incomplete row that is not t0, and next_obs
 * everywhere but at `last` of a trajectory row enter no result and may hold anything, NaN included; the planes must be readable
 * all the same (the call may load any of their elements).  The flag planes and next_row are read at trajectory rows only.
 *
 * (d) Subnormals.  The library is built without -fgpu-flush-denormals-to-zero and without -ffast-math: its kernels run with f32
 * denormals enabled (float_denorm_mode_32 = 3 in every kernel descriptor), so a subnormal p -- gamma = 1e-10 reaches one at
 * m = 4 -- is KEPT, as are subnormal rewards and sums; fmaf and the multiply round them as IEEE 754 does.  -ffp-contract=off: no
 * operation is fused that is not written as fmaf above.
 * (tests/nstep_ref.py, tests/test_nstep_cpu.py, tests/test_gpu_nstep.py)
 */
#ifndef PHANTOM_AMD_NSTEP_H
#define PHANTOM_AMD_NSTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_nstep_io {
  int32_t T;  int32_t D;      /* rows; f32 words per observation (used only when nstep_next_obs != NULL, then 1 <= D <= 64) */
  int64_t N;                  /* columns per row (B * S)                                          */
  int32_t n;  float gamma;    /* 1 <= n <= 64; gamma in [0, 1]                                    */
  const float*   reward;      /* [T][N]  the TRANSITION's reward: phx_gae_masked's reward_sum, or a plain env's reward plane; required */
  const uint8_t* truncated;   /* [T][N]  required: phx_traj_next's next_truncated, or a plain env's truncated plane                    */
  const uint8_t* terminated;  /* [T][N]  or NULL == all zero                                      */
  const uint8_t* acted;       /* [T][N]  or NULL == all one (!= 0: a trajectory row)              */
  const int32_t* next_row;    /* [T][N]  phx_traj_next's next_row, or NULL == "row t itself" (every transition complete) */
  const float*   next_obs;    /* [T][N][D] phx_traj_next's next_obs, or a plain env's observations plane; required iff nstep_next_obs != NULL */
  int32_t* succ_row;          /* [T][N]  output, required iff acted != NULL: the column's next trajectory row after t, -1: none */
  float*   nstep_reward;      /* [T][N]  required */
  float*   nstep_discount;    /* [T][N]  required */
  int32_t* nstep_last;        /* [T][N]  required: the trajectory row of the last transition folded */
  uint8_t* nstep_terminated;  /* [T][N]  required */
  uint8_t* nstep_truncated;   /* [T][N]  required */
  int32_t* nstep_next_row;    /* [T][N]  required */
  float*   nstep_next_obs;    /* [T][N][D] or NULL: no gather */
} phx_nstep_io;               /* 136 bytes */

/* Alignment: the inputs their natural one -- reward, next_row and next_obs 4 bytes, the flag planes none: rows [t0, t1) of a longer
 * recording are fine (next_row then counts rows from t0) -- every output, succ_row included, 16 bytes.  Element offsets are 64-bit:
 * T * N * D may exceed 2^31.  The outputs must not overlap the inputs or each other.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_nstep: io, reward, truncated or one of the six required
 * outputs NULL; acted given without succ_row; nstep_next_obs given without next_obs; D outside [1, 64] when nstep_next_obs is
 * given; T < 1 or N < 1; N beyond one launch's grid (N > 64 * (2^31 - 1), or with nstep_next_obs N * D > 256 * (2^31 - 1)); n
 * outside [1, 64]; gamma outside [0, 1], NaN included; a misaligned pointer.  Nothing is launched then.  PHX_EHIP: a launch failed.
 * The call is up to three launches on `stream`, in this order: phx_nstep_succ_kernel (only with acted), phx_nstep_fold_kernel,
 * phx_nstep_gather_kernel (only with nstep_next_obs).  After a successful call phx_last_kernel() reads the names of the kernels
 * launched joined by "+": "phx_nstep_fold_kernel", "phx_nstep_succ_kernel+phx_nstep_fold_kernel",
 * "phx_nstep_fold_kernel+phx_nstep_gather_kernel" or "phx_nstep_succ_kernel+phx_nstep_fold_kernel+phx_nstep_gather_kernel". */
int phx_nstep(const phx_nstep_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_NSTEP_H */
