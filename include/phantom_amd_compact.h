/*
 * phantom_amd_compact.h -- drop the hole rows of a rollout fragment on the device: a stream compaction of time-major planes, fused
 * with the time-major to agent-major transpose, in one call.
 *
 * A fifth, additive header of libphantom_amd.so: nothing in phantom_amd.h, phantom_amd_gae.h, phantom_amd_vtrace.h or
 * phantom_amd_traj.h changes (PHX_ABI_VERSION stays 10, the return codes and phx_last_error / phx_last_kernel are the ones declared
 * in phantom_amd.h).  Like phx_traj_next the function takes no env handle: planes in, planes out, on the current device,
 * asynchronously on `stream`.
 *
 * On FSM and Stackelberg envs an agent acts in some steps only; a learner reads the rows where it acted.  A column is one (env
 * instance, strategic agent) pair of a phx_rollout fragment, n = b * S + s, N = B * S; row t is step t.  `keep` says which elements
 * (t, n) stay (the fragment's `acted` plane), and every plane of the call is compacted with the same `keep`:
 *
 *   count[n] = the number of rows t with keep[t][n] != 0
 *   start[n] = the sum of count[m] over m < n, as i64;      start[N] = K, the number of kept elements
 *   the position of a kept element (t, n) is  p = start[n] + #{u < t : keep[u][n] != 0}
 *
 * Kept elements are therefore ordered by column, then by row: (env instance, agent, step), the row order of a sample batch.
 * For a kept element with p < capacity
 *
 *   every used plane k:  plane[k].dst[p] = plane[k].src[t][n]      (elem_bytes bytes, COPIED: elements are moved as integers and
 *                                                                   never computed with -- NaN payloads and -0.0 survive)
 *   out_row[p] = t        (when given)
 *   out_col[p] = n        (when given)
 *
 * A kept element with p >= capacity is written nowhere.  `start` is complete whatever `capacity` is: the caller reads K from
 * start[N] and compares.  No byte of a dst, of out_row or of out_col at or beyond element min(K, capacity) is written, and no byte
 * outside start[0 .. N].
 *
 * (a) Reduction.  With every keep byte non-zero each dst is the [N][T] transpose of its src, start[n] = n * T, out_row cycles
 * 0 .. T - 1 and out_col[p] = p / T.
 *
 * (b) Unread elements.  Of a src only the kept elements enter a result; all of it must be readable all the same (the call may load
 * any of its T * N elements).
 * (tests/compact_ref.py, tests/test_compact_cpu.py, tests/test_gpu_compact.py)
 */
#ifndef PHANTOM_AMD_COMPACT_H
#define PHANTOM_AMD_COMPACT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_COMPACT_MAX_PLANES 16

typedef struct phx_compact_plane {
  const void* src;        /* [T][N] elements of elem_bytes bytes, time-major            */
  void*       dst;        /* [capacity] elements of elem_bytes bytes, dense             */
  int32_t elem_bytes;     /* 1, or 4 * w with 1 <= w <= 64 (w 32-bit words per element) */
  int32_t reserved;       /* 0 */
} phx_compact_plane;      /* 24 bytes */

typedef struct phx_traj_compact_io {
  int32_t T;  int32_t n_planes;     /* rows; planes used (0 .. 16: 0 = counts and offsets only) */
  int64_t N;                        /* columns per row (B * S)                                  */
  int64_t capacity;                 /* elements every dst / out_row / out_col can hold (>= 0)   */
  const uint8_t* keep;              /* [T][N] required; != 0 keeps the element                  */
  int64_t* start;                   /* [N + 1] required                                         */
  int32_t* out_row;                 /* [capacity] or NULL                                       */
  int32_t* out_col;                 /* [capacity] or NULL (given: N <= 2^31 - 1)                */
  phx_compact_plane plane[PHX_COMPACT_MAX_PLANES];
} phx_traj_compact_io;              /* 440 bytes */

/* Alignment: keep none, a src its natural one (elem_bytes 1: none, else 4 bytes) -- rows [t0, t1) of a longer recording are
 * fine -- start, out_row, out_col and every dst 16 bytes.  Element offsets are 64-bit: T * N * w may exceed 2^31.  The outputs must
 * not overlap the inputs or each other.  Planes at index n_planes and above are not looked at.
 * Returns PHX_OK, or PHX_EINVAL with a phx_last_error text that names phx_traj_compact: io, keep or start NULL; T < 1 or N < 1;
 * n_planes outside [0, 16]; capacity < 0; a used plane with a NULL src or dst, an elem_bytes that is neither 1 nor 4 * w with
 * 1 <= w <= 64, or reserved != 0; out_col given with N > 2^31 - 1; N beyond one launch's grid (N > 64 * (2^31 - 1)); a misaligned
 * pointer.  Nothing is launched then.  PHX_EHIP: a launch failed.
 * The call is three launches on `stream`: the counts into `start` (which serves as the scratch: no workspace), the exclusive
 * prefix over start[0 .. N] in place, and the scatter.  After a successful call phx_last_kernel() reads
 * "phx_compact_count_kernel+phx_compact_scan_kernel+phx_compact_scatter_kernel"; where the scatter has nothing to write
 * (capacity == 0, or n_planes == 0 with neither out_row nor out_col) it is not launched and the text ends after the scan's name. */
int phx_traj_compact(const phx_traj_compact_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_COMPACT_H */
