/*
 * phantom_amd_filter.h -- a running mean / standard deviation filter of observations on the device (RLlib's
 * observation_filter="MeanStdFilter"): per CLASS of columns (a policy) and per observation feature a running count, mean and M2,
 * folded a rollout fragment at a time in a fixed order -- so the statistics are reproducible bit for bit -- and the pass that hands a
 * learner (x - mean) / (std + 1e-8), clipped.
 *
 * A twelfth, additive header of libphantom_amd.so: nothing in phantom_amd.h or in the other ten additive headers changes
 * (PHX_ABI_VERSION stays 10, the return codes and phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like
 * the others the two functions take no env handle: buffers in, buffers out, on the current device, asynchronously on `stream`.
 *
 * Planes.  `obs` is f32 [T][N][D], time-major: row t is step t, N = B * S columns, the D features of an element contiguous;
 * 1 <= D <= PHX_FILTER_MAX_DIM.  `keep` is u8 [T][N], != 0 keeps the element, NULL keeps all.  `col_class` is i32 [N], the class of
 * every column; NULL: every column is class 0; a value outside [0, n_classes) excludes the column.  1 <= n_classes <=
 * PHX_FILTER_MAX_CLASSES.  Element offsets are 64-bit.
 *
 * State.  phx_filter_state[n_classes] on the device, 272 bytes per class.  All zero: nothing seen; the caller zero-fills it once.
 * mean[d] and m2[d] for d >= D stay as they are (zero after the zero-fill).
 *
 * phx_filter_update folds one fragment into the statistics of all classes.  Kept values must be finite.  Every f64 operation below is
 * the correctly rounded one and none is contracted to an fma (the library is built with -ffp-contract=off).  FOLD(v) of per-column
 * values v_n for class c is the fixed order of phantom_amd_episodes.h:
 *   1. 256 lane values, i = 0 .. 255:  a_i = ((+0.0 + v_i) + v_{i+256}) + v_{i+512} ..., n ascending while n < N, where a column of
 *      another class (or of none) contributes +0.0 -- which is the same as leaving it out;
 *   2. for h = 128, 64, .., 1:  a_i = a_i + a_{i+h} for i < h;
 *   3. the result is a_0.
 * For every class c and feature d:
 *   pass 1, per column n of class c:  s_n = +0.0;  for t = 0 .. T-1 ascending, where kept:  s_n = s_n + (double)x[t][n][d]
 *           K_c = the number of kept elements in the class's columns (an exact integer);  mb = FOLD(s) / (double)K_c
 *   pass 2, per column:               q_n = +0.0;  where kept:  q_n = q_n + ((double)x - mb) * ((double)x - mb)
 *           M2b = FOLD(q)
 *   merge (Chan):  na = count;  n = na + K_c;  delta = mb - mean[d]
 *           mean[d] = mean[d] + delta * ((double)K_c / (double)n)
 *           m2[d]   = (m2[d] + M2b) + (delta * delta) * (((double)na * (double)K_c) / (double)n)
 *   and once per class:  count = n;  updates = updates + 1.
 * A class with K_c == 0 keeps its 272 bytes bit for bit, `updates` included.  The sum of squares is centred in two passes on purpose:
 * a stock level near 1e6 with unit spread keeps its variance, which sumsq / K - mean * mean loses to cancellation.  The statistics
 * are those of the `obs` rows the caller passes: an episode's final new_obs, which no policy acts on, is not in them.
 *
 * Workspace of the update: PHX_FILTER_WORKSPACE_BYTES(N, D) bytes, 16-byte aligned, scratch (the per-column partials and a table
 * per class and feature); its contents mean nothing between calls.
 *
 * phx_filter_apply normalises a plane with the state as it stands and never writes the state.  Per class and feature:
 *   count == 0:  mean_f = +0.0f, den_f = 1.0f, and NO clip: the identity, kept values are copied bit for bit;
 *   count == 1:  var = mean * mean        (RLlib's RunningStat.var);
 *   otherwise:   var = m2 / (double)(count - 1);
 *   then         mean_f = (float)mean,  den_f = (float)sqrt(var) + 1e-8f   (the sum in f32).
 * Per element of `out` (f32 [T][N][D], EVERY element is written):
 *   kept, in a column with a class:  y = (x - mean_f) / den_f, two correctly rounded f32 operations; with clip > 0 and count > 0
 *                                    then y = fminf(fmaxf(y, -clip), clip);
 *   otherwise:                       +0.0f.
 * out == obs (exactly in place) is allowed; any other overlap is refused.  `clip` must be >= 0; 0: none.
 *
 * Folding the filter into a network's first layer (host code, ObsFilter.fold; the rollout kernels then act on raw observations):
 * from mean_f / den_f as above, W'[j][i] = (float)((double)W[j][i] / (double)den_f[i]) and b'[j] = (float)((double)b[j] - sum), sum
 * running over i ascending from +0.0 of ((double)W[j][i] * (double)mean_f[i]) / (double)den_f[i].  A clipped filter cannot be folded.
 *
 * Known answers (tests/test_filter_cpu.py): N = 5, T = 3, D = 2, n_classes = 2, col_class = 0 1 0 1 0, keep NULL,
 * x[t][n][d] = (float)(((u * 7 + 3 * t + 5 * n + 11 * d) % 13) - 4) / 2 for update u = 0, 1, 2.  After the three updates:
 *   class 0: count 27, updates 3, mean 0.537037037037037 1.4629629629629628, m2 94.46296296296296 94.46296296296296
 *   class 1: count 18, updates 3, mean 1.5 0.5, m2 52.5 52.5
 * (tests/filter_ref.py, tests/test_filter_cpu.py, tests/test_gpu_filter.py)
 */
#ifndef PHANTOM_AMD_FILTER_H
#define PHANTOM_AMD_FILTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_FILTER_MAX_DIM 16
#define PHX_FILTER_MAX_CLASSES 16
/* the update's workspace in bytes: (D + 1) * N per-column words and a table of 528 */
#define PHX_FILTER_WORKSPACE_BYTES(N, D) (8 * (((int64_t)(D) + 1) * (int64_t)(N) + 528))

typedef struct phx_filter_state {
  int64_t count;  int64_t updates;       /* 0, 8    kept elements folded so far; updates that folded at least one */
  double  mean[PHX_FILTER_MAX_DIM];      /* 16      the running mean of every feature                             */
  double  m2[PHX_FILTER_MAX_DIM];        /* 144     the running sum of squared deviations from it                 */
} phx_filter_state;                      /* 272 bytes */

typedef struct phx_filter_update_io {
  int32_t T;  int32_t D;                 /* 0, 4    rows; features per element, 1 <= D <= 16 */
  int64_t N;                             /* 8       columns                                  */
  int32_t n_classes;  int32_t reserved0; /* 16, 20  1 <= n_classes <= 16; 0                  */
  const float*   obs;                    /* 24      [T][N][D] required                       */
  const uint8_t* keep;                   /* 32      [T][N] or NULL == all kept               */
  const int32_t* col_class;              /* 40      [N] or NULL == all class 0               */
  phx_filter_state* state;               /* 48      [n_classes] in/out                       */
  double* workspace;                     /* 56      PHX_FILTER_WORKSPACE_BYTES(N, D) bytes   */
  int64_t reserved[2];                   /* 64      0                                        */
} phx_filter_update_io;                  /* 80 bytes */

typedef struct phx_filter_apply_io {
  int32_t T;  int32_t D;                 /* 0, 4 */
  int64_t N;                             /* 8 */
  int32_t n_classes;  float clip;        /* 16, 20  clip >= 0; 0: none                       */
  const float*   obs;                    /* 24      [T][N][D] required                       */
  const uint8_t* keep;                   /* 32      [T][N] or NULL == all kept               */
  const int32_t* col_class;              /* 40      [N] or NULL == all class 0               */
  const phx_filter_state* state;         /* 48      [n_classes], read only                   */
  float* out;                            /* 56      [T][N][D] required; may equal obs        */
  int64_t reserved[2];                   /* 64      0                                        */
} phx_filter_apply_io;                   /* 80 bytes */

/* Alignment: obs, out, state and workspace 16 bytes, col_class 4 bytes, keep none (rows [t0, t1) of a longer recording are fine).
 * Both return PHX_OK, or PHX_EINVAL with a phx_last_error text that names the function, and then launch nothing: io NULL; obs or
 * state NULL; (update) workspace NULL; (apply) out NULL; a misaligned pointer; T < 1 or N < 1; D or n_classes outside [1, 16];
 * (apply) clip negative or NaN; (apply) out overlapping obs in part; a non-zero reserved field; sizes beyond one launch's grid:
 * (update) N > 64 * (2^31 - 1), (apply) N * D > 2^31 - 1 - 4096 or T * N * D > 4096 * (2^31 - 1).  PHX_EHIP: a launch failed.
 * phx_filter_update is five launches on `stream`; after a successful call phx_last_kernel() reads
 * "phx_filter_sum_kernel+phx_filter_mean_kernel+phx_filter_center_kernel+phx_filter_m2_kernel+phx_filter_merge_kernel".
 * phx_filter_apply is one launch; phx_last_kernel() then reads "phx_filter_apply_kernel". */
int phx_filter_update(const phx_filter_update_io* io, void* stream);
int phx_filter_apply(const phx_filter_apply_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_FILTER_H */
