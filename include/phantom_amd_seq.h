/*
 * phantom_amd_seq.h -- a recurrent or attention learner's batch from the time-major planes of a rollout fragment, on the device: every
 * column's kept rows cut into SEQUENCES at episode ends and every max_seq_len rows, each sequence zero-padded to max_seq_len, one
 * column standardized and the sequences (not the rows) shuffled -- RLlib's chop_into_sequences, written as records, in one call.
 *
 * A ninth, additive header of libphantom_amd.so: nothing in the other eight changes (PHX_ABI_VERSION stays 10, the return codes and
 * phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  phx_batch_plane, phx_batch_moments and
 * PHX_BATCH_MAX_PLANES are phantom_amd_batch.h's.  The function takes no env handle: planes in, buffers out, on the current device,
 * asynchronously on `stream`.
 *
 * Kept elements.  phantom_amd_batch.h's rule: a column is one (env instance, strategic agent) pair, n = b * S + s, row t is step t,
 * and element (t, n) is KEPT iff
 *
 *   (keep == NULL || keep[t][n] != 0) && (col_class == NULL || col_class[n % S] == class_id)
 *
 * Sequences.  L = max_seq_len, 1 <= L <= 65536.  `terminated` and `truncated` are u8 [T][N] planes, each may be NULL (all zero); they
 * are read at kept elements only: what they hold elsewhere does not matter.  Every column n is walked on its own, t ascending,
 * carrying len = 0 and g = 0.  At every kept row:
 *
 *   1. if len == 0, sequence (n, g) opens here: first_row = t
 *   2. the row's position in its sequence is i = len
 *   3. len += 1
 *   4. if terminated[t][n] != 0 || truncated[t][n] != 0 || len == L: the sequence closes with seq_len = len; g += 1; len = 0
 *
 * After row T - 1 an open sequence (len > 0) closes with seq_len = len.  A cut on the L-th row closes one sequence, not two; no
 * sequence is empty.
 *
 *   Q_n = the number of sequences of column n
 *   seq_start[n] = the sum of Q_m over m < n, as i64;      seq_start[N] = Q, the number of sequences
 *
 * `seq_start` is complete whatever else happens.
 *
 * Permutation.  A sequence's index is s = seq_start[n] + g.  sigma = s when shuffle == 0 or Q <= 1; otherwise sigma = perm_Q(s),
 * phantom_amd_batch.h's cycle-walking Feistel bijection with the round keys of (seed, epoch) and Q in the place of K.
 *
 * Outputs.  If Q > capacity (capacity counts SEQUENCES) nothing but `seq_start` (and `moments`) is written.  Otherwise, for a kept
 * element at position i of sequence s, its SLOT is sigma * L + i and
 *
 *   records[slot * row_words + ..]   phantom_amd_batch.h's record: plane words copied as integers, a byte plane zero-extended to one
 *                                    word, words that no plane covers 0
 *   out_row[slot] = t,  out_col[slot] = n                                                       (when given)
 *   every PADDING slot sigma * L + i, seq_len <= i < L: all row_words words 0, out_row = -1, out_col = -1
 *   seq_lens[sigma] = seq_len,  seq_row[sigma] = first_row,  seq_col[sigma] = n                 (each optional, i32)
 *
 * Every slot below Q * L is written exactly once.  No byte of records / out_row / out_col at or beyond slot Q * L and no byte of
 * seq_lens / seq_row / seq_col at or beyond sequence Q is written.
 *
 * Standardization.  With std_plane >= 0 the rule is phantom_amd_batch.h's to the letter: the f64 sums per column over kept elements
 * in row order, the fixed 256-lane fold over columns, moments.count = K -- the kept ROWS, not the padded slots -- and the same mean
 * and den.  The standardized word is stored at kept slots only; padding stays 0.
 * (tests/seq_ref.py, tests/test_seq_batch_cpu.py, tests/test_gpu_seq_batch.py)
 */
#ifndef PHANTOM_AMD_SEQ_H
#define PHANTOM_AMD_SEQ_H

#include <stdint.h>

#include "phantom_amd_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_SEQ_MAX_LEN 65536

typedef struct phx_seq_batch_io {
  int64_t T;                        /* 0    rows, 1 <= T <= 2^31 - 1                                             */
  int64_t N;                        /* 8    columns per row (B * S); T * N <= 2^62                               */
  int64_t capacity;                 /* 16   SEQUENCES the outputs can hold (>= 0); capacity * max_seq_len <= 2^62 */
  int32_t n_planes;                 /* 24   planes used (0 .. 32)                                                */
  int32_t row_words;                /* 28   32-bit words per record: a multiple of 4 in [4, 256]                 */
  int32_t S;                        /* 32   entries of col_class, S >= 1 and N % S == 0 (also without it)        */
  int32_t class_id;                 /* 36   the class this call keeps                                            */
  int32_t std_plane;                /* 40   -1, or the index of a 4-byte plane holding f32                       */
  int32_t shuffle;                  /* 44   0 or 1                                                               */
  uint64_t seed;                    /* 48                                                                        */
  uint64_t epoch;                   /* 56                                                                        */
  const uint8_t* keep;              /* 64   [T][N], or NULL: every element                                       */
  const uint8_t* col_class;         /* 72   [S], or NULL: every column is in the class                           */
  int64_t* seq_start;               /* 80   [N + 1] required                                                     */
  uint32_t* records;                /* 88   [capacity][max_seq_len][row_words]; required with n_planes > 0 (and room) */
  int32_t* out_row;                 /* 96   [capacity][max_seq_len] or NULL                                      */
  int32_t* out_col;                 /* 104  [capacity][max_seq_len] or NULL (given: N <= 2^31 - 1)               */
  phx_batch_moments* moments;       /* 112  one record; required with std_plane >= 0 (written only then)         */
  void* workspace;                  /* 120  24 * N bytes; required with std_plane >= 0                           */
  int64_t max_seq_len;              /* 128  L, 1 <= L <= 65536                                                   */
  const uint8_t* terminated;        /* 136  [T][N], or NULL: all zero                                            */
  const uint8_t* truncated;         /* 144  [T][N], or NULL: all zero                                            */
  int32_t* seq_lens;                /* 152  [capacity] or NULL                                                   */
  int32_t* seq_row;                 /* 160  [capacity] or NULL                                                   */
  int32_t* seq_col;                 /* 168  [capacity] or NULL (given: N <= 2^31 - 1)                            */
  int64_t reserved[2];              /* 176  0                                                                    */
  phx_batch_plane plane[PHX_BATCH_MAX_PLANES];      /* 192 */
} phx_seq_batch_io;                 /* 704 bytes */

/* Alignment: keep, terminated, truncated, col_class and byte planes none, a word plane's src 4 bytes -- rows [t0, t1) of a longer
 * recording are fine -- seq_start, records, out_row, out_col, seq_lens, seq_row, seq_col, moments and workspace 16 bytes.  Element
 * offsets are 64-bit.  The outputs must not overlap the inputs or each other.  Planes at index n_planes and above are not looked at.
 * All of a src, and of keep / terminated / truncated, must be readable (the call may load any of the T * N elements).
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_seq_batch: io or seq_start NULL; records NULL with
 * n_planes > 0 and capacity > 0; T < 1, T > 2^31 - 1, N < 1, T * N > 2^62, S < 1 or N % S != 0; max_seq_len outside [1, 65536];
 * capacity < 0 or capacity * max_seq_len > 2^62; n_planes outside [0, 32]; a used plane with a NULL src or an elem_bytes that is
 * neither 1 nor 4 * w with 1 <= w <= 64; row_words not a multiple of 4 in [4, 256]; a plane's words outside the record or overlapping
 * another plane's; std_plane outside [-1, n_planes) or naming a plane whose elem_bytes is not 4; moments or workspace NULL with
 * std_plane >= 0; shuffle neither 0 nor 1; a non-zero reserved field; out_col or seq_col given with N > 2^31 - 1; N beyond one
 * launch's grid (N > 64 * (2^31 - 1)); a misaligned pointer.  Nothing is launched then.  PHX_EHIP: a launch failed.
 * The call is up to four launches on `stream`: phx_seq_count_kernel (Q_n into `seq_start`; with std_plane the per-column sums and
 * kept rows into `workspace`), phx_seq_scan_kernel (the exclusive prefix over seq_start[0 .. N] in place), phx_seq_moments_kernel
 * (only with std_plane >= 0) and phx_seq_scatter_kernel (records, indices, the per-sequence outputs and the padding; not launched
 * where it has nothing to write: capacity == 0, or records, out_row, out_col, seq_lens, seq_row and seq_col all NULL).  After a
 * successful call phx_last_kernel() reads the names of the kernels launched joined with "+", in that order:
 * "phx_seq_count_kernel+phx_seq_scan_kernel+phx_seq_moments_kernel+phx_seq_scatter_kernel" with all four. */
int phx_seq_batch(const phx_seq_batch_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_SEQ_H */
