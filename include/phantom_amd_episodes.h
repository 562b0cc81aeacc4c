/*
 * phantom_amd_episodes.h -- episode returns and lengths of a rollout fragment (RLlib's episode_reward_mean / min / max,
 * episode_len_mean, episodes_this_iter, policy_reward_mean): a forward scan over the fragment's rows with a carry per output column,
 * so that an episode a fragment cuts is finished by the next call, over trajectories with holes as well, and a fixed-order reduction
 * of the per-column statistics into per-class ones.
 *
 * A seventh, additive header of libphantom_amd.so: nothing in phantom_amd.h, phantom_amd_gae.h, phantom_amd_vtrace.h,
 * phantom_amd_traj.h, phantom_amd_compact.h or phantom_amd_nstep.h changes (PHX_ABI_VERSION stays 10, the return codes and
 * phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like the other six the function takes no env handle:
 * planes in, planes out, on the current device, asynchronously on `stream`.
 *
 * Columns, groups and classes.  The inputs are time-major planes [T][N] of a phx_rollout fragment: N = B * S input columns, row t is
 * step t.  An OUTPUT column c is a group of G consecutive input columns n = c * G + g, g = 0 .. G - 1; C = N / G.  G = 1: one output
 * column per (env instance, agent); G = S: one per env instance, RLlib's episode.  Output columns fall into K CLASSES, k = c % K:
 * K = S with G = 1 gives per-agent statistics over the batch, K = 1 with G = S one statistic over all env instances.
 *
 * The scan runs per output column c, forward in t.  Its state is ret (f32) and len (i32, -1: no episode is open), read from
 * carry_return[c] / carry_len[c] when the carry is given, else ret = +0.0f, len = -1.  Every operation is the correctly rounded f32
 * (f64 where written) one; the library is built with -ffp-contract=off.
 *
 *   for t = 0 .. T-1:
 *     any_act = false; all_flag = true
 *     for g = 0 .. G-1 (ascending), n = c*G + g, o = t*N + n:
 *       present = reward_valid == NULL || reward_valid[o] == 1          (only the value 1 counts, as in phx_gae_masked)
 *       act     = acted == NULL || acted[o] != 0
 *       if (present || act) and len < 0: ret = +0.0f; len = 0          (an episode OPENS)
 *       if present: ret = ret + reward[o]
 *       any_act |= act
 *       all_flag &= (terminated != NULL && terminated[o] != 0) || truncated[o] != 0
 *     if any_act: len += 1
 *     if all_flag && len >= 0:   an episode CLOSES at row t with (ret, len):
 *          episode_return[t][c] = ret; episode_len[t][c] = len
 *          col.count += 1; col.len_sum += len; col.len_min / len_max updated
 *          col.ret_sum   = col.ret_sum   + (double)ret                   (f64, in t order, from +0.0)
 *          col.ret_sumsq = col.ret_sumsq + (double)ret * (double)ret     (the product of two converted f32 values is exact in f64)
 *          col.ret_min / ret_max updated by value
 *          ret = +0.0f; len = -1
 *     else: episode_return[t][c] = +0.0f; episode_len[t][c] = -1
 *   after row T-1: carry_return[c] = ret; carry_len[c] = len   (when the carry is given: read and written in place)
 *
 * A flagged row with nothing open closes nothing: an agent that terminated earlier and merely sees the env's truncation, or sticky
 * flags, count no second episode.  `reward` where present is false enters no result and may hold anything, NaN included (the plane
 * must be readable all the same); present rewards must be finite.  Both per-row planes are optional; when given they are written
 * everywhere.
 *
 * col_stats[c] covers THIS CALL only: it starts empty on every call, whatever the carry holds (an episode the carry brought in and
 * this call closes counts here, with its whole return and length).  Empty: count = len_sum = 0, both sums +0.0, ret_min = +inf,
 * ret_max = -inf, len_min = INT32_MAX, len_max = -1.  Where +0.0 and -0.0 tie in ret_min / ret_max either may be stored.
 *
 * Reduction.  summary[k] combines the M = C / K columns c = j * K + k, j = 0 .. M - 1.  The integer fields are the exact sums / min /
 * max, ret_min / ret_max combine by value, and each of the two f64 sums is taken in this fixed order:
 *   1. 256 lane values, i = 0 .. 255:  a_i = ((+0.0 + x_i) + x_{i+256}) + x_{i+512} ..., j ascending while j < M;
 *   2. for h = 128, 64, .., 1:  a_i = a_i + a_{i+h} for i < h;
 *   3. the result is a_0.
 * (tests/episode_ref.py, tests/test_episode_stats_cpu.py, tests/test_gpu_episode_stats.py)
 */
#ifndef PHANTOM_AMD_EPISODES_H
#define PHANTOM_AMD_EPISODES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One element of col_stats[C] and of summary[K].  The tag shares its name with the function below, so the type is written with the
 * `struct` keyword (a typedef of that name would collide with the function in C). */
struct phx_episode_stats {
  int64_t count;  int64_t len_sum;       /* 0, 8   episodes closed; the sum of their lengths */
  double  ret_sum; double ret_sumsq;     /* 16, 24 the sum of their returns and of the returns' squares */
  float   ret_min; float  ret_max;       /* 32, 36 */
  int32_t len_min; int32_t len_max;      /* 40, 44 */
};                                        /* 48 bytes */

typedef struct phx_episode_io {
  int32_t T;  int32_t G;                 /* 0, 4    rows; input columns per output column, 1 <= G <= 256 */
  int64_t N;                             /* 8       input columns, N % G == 0                             */
  int32_t K;  int32_t reserved0;         /* 16, 20  classes, K >= 1, (N / G) % K == 0; 0                  */
  const float*   reward;                 /* 24      [T][N] required                                       */
  const uint8_t* truncated;              /* 32      [T][N] required                                       */
  const uint8_t* terminated;             /* 40      [T][N] or NULL == all zero                            */
  const uint8_t* acted;                  /* 48      [T][N] or NULL == all one                             */
  const uint8_t* reward_valid;           /* 56      [T][N] or NULL == all one; only 1 counts              */
  float*   carry_return;                 /* 64      [C] in/out, or NULL                                   */
  int32_t* carry_len;                    /* 72      [C] in/out; given iff carry_return is                 */
  float*   episode_return;               /* 80      [T][C] or NULL                                        */
  int32_t* episode_len;                  /* 88      [T][C] or NULL                                        */
  struct phx_episode_stats* col_stats;   /* 96      [C] required                                          */
  struct phx_episode_stats* summary;     /* 104     [K] or NULL: no reduction launch                      */
} phx_episode_io;                        /* 112 bytes */

/* Alignment: the inputs their natural one -- reward 4 bytes, the flag planes none: rows [t0, t1) of a longer recording are fine --
 * the two carry arrays 4 bytes, the four output planes and arrays (episode_return, episode_len, col_stats, summary) 16 bytes.
 * Element offsets are 64-bit: T * N may exceed 2^31.  The outputs must not overlap the inputs or each other.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_episode_stats: io, reward, truncated or col_stats NULL;
 * exactly one of carry_return / carry_len given; T < 1 or N < 1; G outside [1, 256]; N % G != 0; K < 1; (N / G) % K != 0;
 * reserved0 != 0; C beyond one launch's grid (C > 64 * (2^31 - 1)); a misaligned pointer.  Nothing is launched then.  A carry_len
 * below -1 is device data and is not checked (it reads as "no episode open").  PHX_EHIP: a launch failed.
 * The call is one launch on `stream`, phx_episode_scan_kernel, or two with `summary`, phx_episode_reduce_kernel after it.  After a
 * successful call phx_last_kernel() reads "phx_episode_scan_kernel" or "phx_episode_scan_kernel+phx_episode_reduce_kernel". */
int phx_episode_stats(const phx_episode_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_EPISODES_H */
