/*
 * phantom_amd_batch.h -- a learner's batch from the time-major planes of a rollout fragment, on the device: hole rows dropped, rows in
 * (env instance, agent, step) order, one policy's columns selected, one column standardized (RLlib's
 * standardize_fields=["advantages"]) and the rows shuffled -- written as RECORDS, all columns of a row contiguous, in one call.
 *
 * An eighth, additive header of libphantom_amd.so: nothing in phantom_amd.h, phantom_amd_gae.h, phantom_amd_vtrace.h,
 * phantom_amd_traj.h, phantom_amd_compact.h, phantom_amd_nstep.h or phantom_amd_episodes.h changes (PHX_ABI_VERSION stays 10, the
 * return codes and phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like the other seven the function takes
 * no env handle: planes in, buffers out, on the current device, asynchronously on `stream`.
 *
 * Kept elements.  A column is one (env instance, strategic agent) pair, n = b * S + s; row t is step t.  Element (t, n) is KEPT iff
 *
 *   (keep == NULL || keep[t][n] != 0) && (col_class == NULL || col_class[n % S] == class_id)
 *
 * One call serves one class (one policy); a caller with P policies makes P calls.
 *
 * Positions are phx_traj_compact's:
 *
 *   count[n] = the number of kept rows of column n
 *   start[n] = the sum of count[m] over m < n, as i64;      start[N] = K, the number of kept elements
 *   p = start[n] + #{u < t : (u, n) kept}
 *
 * `start` is complete whatever else happens.
 *
 * Permutation.  q = p when shuffle == 0 or K <= 1.  Otherwise q = perm_K(p), a cycle-walking Feistel bijection on [0, K) in integer
 * arithmetic only.  w is the smallest even integer >= 2 with 2^w >= K, h = w / 2, mask = 2^h - 1.  Six 32-bit round keys come from
 * splitmix64 (all arithmetic mod 2^64):
 *
 *   s = seed ^ (epoch * 0x9E3779B97F4A7C15)
 *   for r = 0 .. 5:  s += 0x9E3779B97F4A7C15;  z = s;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                    z ^= z >> 31;  key[r] = (uint32_t)z
 *
 * The round function on u32:   x = R ^ key[r];  x *= 0x9E3779B1; x ^= x >> 15;  x *= 0x85EBCA77; x ^= x >> 13;
 *                              x *= 0xC2B2AE3D; x ^= x >> 16;  F_r(R) = x & mask
 * The walk:   x = p
 *             do { L = x >> h; R = x & mask;  for r = 0 .. 5: (L, R) = (R, L ^ F_r(R));  x = (L << h) | R; } while (x >= K);
 *             q = x
 *
 * The six rounds are a permutation of [0, 2^w) (each round is invertible), so p lies on a cycle of it; following the cycle from p,
 * the first value below K is reached before p comes round again (p itself is below K): the walk ends, and distinct p end at
 * distinct q.  2^w < 4 K, so the expected trip count 2^w / K is below 4.  T * N <= 2^62 is required (w <= 62).
 *
 * Records.  If K > capacity nothing but `start` (and `moments`) is written: a permutation of [0, K) cannot be clipped; the caller
 * reads start[N] and compares.  Otherwise, for every kept element,
 *
 *   records[q * row_words + plane[k].word_off + j] = word j of plane k's element, COPIED as integers (NaN payloads and -0.0 survive);
 *                                                    a byte plane stores its byte zero-extended to one u32 word
 *   words of the record that no plane covers = 0
 *   out_row[q] = t,  out_col[q] = n                 (when given)
 *
 * No byte of records / out_row / out_col at or beyond record K is written.  A learner reads a column as a strided view of `records`.
 *
 * Standardization.  With std_plane >= 0 (a plane of elem_bytes 4 holding f32), per column n, in ascending t over kept elements only,
 * from +0.0:  s_n += (double)x;  q_n += (double)x * (double)x  (columns that keep nothing contribute +0.0).  The two sums over
 * n = 0 .. N - 1 are taken in phantom_amd_episodes.h's fixed order: 256 lane values a_i folding n = i, i + 256, .. ascending from +0.0,
 * then a_i = a_i + a_{i+h} for i < h, h = 128, 64, .. 1; the result is a_0.  Then, in correctly rounded f64 / f32 operations,
 *
 *   count = K;  m = sum / (double)K;  v = sumsq / (double)K - m * m, a v that is not > 0 becomes 0
 *   mean = (float)m;  den = max(1e-4f, (float)sqrt(v))                 K = 0: (0, +0.0, +0.0, +0.0f, 1e-4f)
 *
 * and the word stored for that plane is the bit pattern of (x - mean) / den, two correctly rounded f32 operations.  Kept values of
 * that plane must be finite.  Every other plane is copied bit for bit.
 * (tests/batch_ref.py, tests/test_train_batch_cpu.py, tests/test_gpu_train_batch.py)
 */
#ifndef PHANTOM_AMD_BATCH_H
#define PHANTOM_AMD_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_BATCH_MAX_PLANES 32

typedef struct phx_batch_plane {
  const void* src;        /* 0   [T][N] elements of elem_bytes bytes, time-major                      */
  int32_t elem_bytes;     /* 8   1, or 4 * w with 1 <= w <= 64 (w 32-bit words per element)           */
  int32_t word_off;       /* 12  the element's first word inside a record (a byte plane covers one)   */
} phx_batch_plane;        /* 16 bytes */

typedef struct phx_batch_moments {
  int64_t count;          /* 0   K                                   */
  double  sum;            /* 8   of the kept values of std_plane     */
  double  sumsq;          /* 16  of their squares                    */
  float   mean;           /* 24                                      */
  float   den;            /* 28  max(1e-4f, the standard deviation)  */
} phx_batch_moments;      /* 32 bytes */

typedef struct phx_train_batch_io {
  int64_t T;                        /* 0    rows, 1 <= T <= 2^31 - 1                                       */
  int64_t N;                        /* 8    columns per row (B * S); T * N <= 2^62                         */
  int64_t capacity;                 /* 16   records that records / out_row / out_col can hold (>= 0)       */
  int32_t n_planes;                 /* 24   planes used (0 .. 32)                                          */
  int32_t row_words;                /* 28   32-bit words per record: a multiple of 4 in [4, 256]           */
  int32_t S;                        /* 32   entries of col_class, S >= 1 and N % S == 0 (also without it)  */
  int32_t class_id;                 /* 36   the class this call keeps                                      */
  int32_t std_plane;                /* 40   -1, or the index of a 4-byte plane holding f32                 */
  int32_t shuffle;                  /* 44   0 or 1                                                         */
  uint64_t seed;                    /* 48                                                                  */
  uint64_t epoch;                   /* 56                                                                  */
  const uint8_t* keep;              /* 64   [T][N], or NULL: every element                                 */
  const uint8_t* col_class;         /* 72   [S], or NULL: every column is in the class                     */
  int64_t* start;                   /* 80   [N + 1] required                                               */
  uint32_t* records;                /* 88   [capacity][row_words]; required with n_planes > 0 (and room)   */
  int32_t* out_row;                 /* 96   [capacity] or NULL                                             */
  int32_t* out_col;                 /* 104  [capacity] or NULL (given: N <= 2^31 - 1)                      */
  phx_batch_moments* moments;       /* 112  one record; required with std_plane >= 0 (written only then)  */
  void* workspace;                  /* 120  16 * N bytes; required with std_plane >= 0                     */
  int64_t reserved[2];              /* 128  0                                                              */
  phx_batch_plane plane[PHX_BATCH_MAX_PLANES];      /* 144 */
} phx_train_batch_io;               /* 656 bytes */

/* Alignment: keep, col_class and byte planes none, a word plane's src 4 bytes -- rows [t0, t1) of a longer recording are fine --
 * start, records, out_row, out_col, moments and workspace 16 bytes.  Element offsets are 64-bit.  The outputs must not overlap the
 * inputs or each other.  Planes at index n_planes and above are not looked at.  All of a src must be readable (the call may load any
 * of its T * N elements).  `moments` is written only with std_plane >= 0.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_train_batch: io or start NULL; records NULL with
 * n_planes > 0 and capacity > 0; T < 1, T > 2^31 - 1, N < 1, T * N > 2^62, S < 1 or N % S != 0; n_planes outside [0, 32]; a used plane with a NULL src
 * or an elem_bytes that is neither 1 nor 4 * w with 1 <= w <= 64; row_words not a multiple of 4 in [4, 256]; a plane's words outside
 * the record or overlapping another plane's; capacity < 0; std_plane outside [-1, n_planes) or naming a plane whose elem_bytes is
 * not 4; moments or workspace NULL with std_plane >= 0; shuffle neither 0 nor 1; a non-zero reserved field; out_col given with
 * N > 2^31 - 1; N beyond one launch's grid (N > 64 * (2^31 - 1)); a misaligned pointer.  Nothing is launched then.  PHX_EHIP: a
 * launch failed.
 * The call is up to four launches on `stream`: phx_batch_count_kernel (the counts into `start`, the per-column sums into
 * `workspace`), phx_batch_scan_kernel (the exclusive prefix over start[0 .. N] in place), phx_batch_moments_kernel (only with
 * std_plane >= 0) and phx_batch_scatter_kernel (not launched where it has nothing to write: capacity == 0, or records, out_row and
 * out_col all NULL).  After a successful call phx_last_kernel() reads the names of the kernels launched joined with "+", in that
 * order: "phx_batch_count_kernel+phx_batch_scan_kernel+phx_batch_moments_kernel+phx_batch_scatter_kernel" with all four. */
int phx_train_batch(const phx_train_batch_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_BATCH_H */
