// phx_frag.h -- the host side that the learner-side entry points over rollout fragments share: phx_gae .. phx_filter_apply, sixteen
// extern "C" functions `(io struct *, stream) -> status` in twelve files.  An entry point is
//   1. its checks, in the order its header states them and all of them before the first HIP call.  A rule that more than one entry
//      point has is a checker here: it takes the entry point's name and returns PHX_OK or what fail(PHX_EINVAL, ..) returned, and the
//      caller writes `if (const int rc = frag_..(fn, ..)) return rc;`.  A rule of one entry point stays in that entry point;
//   2. its launches, each followed by FragCall::launched().
// Host functions only: nothing in this file is compiled for the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "phx_spec.h"

// one call of one entry point
struct FragCall {
  const char* fn;                        // "phx_vtrace"
  bool noted = false;
  // after a hipLaunchKernelGGL: PHX_OK, or PHX_EHIP with "<fn>: <what>: <hip text>" ("<fn>: <hip text>" when `what` is NULL).  The
  // first success of a call resets phx_last_kernel's list and every success appends `kernel`: a call whose first launch fails inside
  // HIP leaves the list of the call before it, as a refused call does.
  int launched(const char* what, const char* kernel) {
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess)
      return what ? fail(PHX_EHIP, "%s: %s: %s", fn, what, hipGetErrorString(he)) : fail(PHX_EHIP, "%s: %s", fn, hipGetErrorString(he));
    if (!noted) phx_note_reset();
    noted = true;
    phx_note_kernel(kernel);
    return PHX_OK;
  }
};

// ---- scalars ----------------------------------------------------------------------------------------------------------------------
inline int frag_io(const char* fn, const void* io) { return io ? PHX_OK : fail(PHX_EINVAL, "%s: null io", fn); }
inline int frag_rows_cols(const char* fn, const int64_t T, const int64_t N) {
  return T >= 1 && N >= 1 ? PHX_OK : fail(PHX_EINVAL, "%s: T = %lld and N = %lld must be >= 1", fn, (long long)T, (long long)N);
}
inline bool frag_unit(const float x) { return x >= 0.0f && x <= 1.0f; }      // in [0, 1] (NaN fails)
inline int frag_gamma_lambda(const char* fn, const float gamma, const float lambda) {
  if (frag_unit(gamma) && frag_unit(lambda)) return PHX_OK;
  return fail(PHX_EINVAL, "%s: gamma = %g and lambda = %g must lie in [0, 1]", fn, (double)gamma, (double)lambda);
}
inline int frag_at_least(const char* fn, const char* name, const int64_t value, const int64_t least) {
  return value >= least ? PHX_OK : fail(PHX_EINVAL, "%s: %s = %lld must be >= %lld", fn, name, (long long)value, (long long)least);
}
// the refusal of what one launch's grid (2^31 - 1 workgroups) does not hold; `subject` (a printf format) says what that is, verb included
__attribute__((format(printf, 2, 3))) inline int frag_beyond_grid(const char* fn, const char* subject, ...) {
  char text[160];
  va_list ap;
  va_start(ap, subject);
  vsnprintf(text, sizeof text, subject, ap);
  va_end(ap);
  return fail(PHX_EINVAL, "%s: %s beyond one launch's grid", fn, text);
}
// `count` items named `name`, `per_group` of them a workgroup
inline int frag_one_grid(const char* fn, const char* name, const int64_t count, const int64_t per_group) {
  return count <= per_group * 0x7fffffffLL ? PHX_OK : frag_beyond_grid(fn, "%s = %lld is", name, (long long)count);
}
inline int frag_reserved0(const char* fn, const int32_t reserved0) { return reserved0 == 0 ? PHX_OK : fail(PHX_EINVAL, "%s: reserved0 must be 0", fn); }
// the struct's reserved[2], with its reserved0 where it has one
inline int frag_reserved(const char* fn, const int64_t (&reserved)[2], const int32_t reserved0 = 0, const char* what = "reserved") {
  return reserved0 == 0 && reserved[0] == 0 && reserved[1] == 0 ? PHX_OK : fail(PHX_EINVAL, "%s: %s must be 0", fn, what);
}
inline int frag_row_words(const char* fn, const int row_words) {
  if (row_words >= 4 && row_words <= 256 && !(row_words & 3)) return PHX_OK;
  return fail(PHX_EINVAL, "%s: row_words = %d must be a multiple of 4 in [4, 256]", fn, row_words);
}
// a record count the host states (count_ptr == NULL) lies in the source; one on the device is checked by the kernels
inline int frag_count(const char* fn, const void* count_ptr, const int64_t count, const int64_t src_capacity) {
  if (count_ptr || (count >= 0 && count <= src_capacity)) return PHX_OK;
  return fail(PHX_EINVAL, "%s: count = %lld must lie in [0, src_capacity = %lld]", fn, (long long)count, (long long)src_capacity);
}

// ---- pointers ---------------------------------------------------------------------------------------------------------------------
inline int frag_required(const char* fn, const bool all_given, const char* names) {
  return all_given ? PHX_OK : fail(PHX_EINVAL, "%s: %s are required", fn, names);
}
// the address bits of some pointers OR-ed (NULL adds none), for frag_aligned
template <typename... P>
inline uintptr_t frag_bits(const P*... p) { return (uintptr_t(0) | ... | (uintptr_t)p); }
inline int frag_aligned(const char* fn, const uintptr_t bits, const unsigned bytes, const char* names) {
  return bits & (bytes - 1u) ? fail(PHX_EINVAL, "%s: %s must be %u-byte aligned", fn, names, bytes) : PHX_OK;
}

// ---- source planes (phx_traj_compact, phx_train_batch, phx_seq_batch) ---------------------------------------------------------------
inline int frag_n_planes(const char* fn, const int n_planes, const int most) {
  return n_planes >= 0 && n_planes <= most ? PHX_OK : fail(PHX_EINVAL, "%s: n_planes = %d must lie in [0, %d]", fn, n_planes, most);
}
inline int frag_plane_elem(const char* fn, const int k, const int elem_bytes) {
  if (elem_bytes == 1 || (elem_bytes >= 4 && elem_bytes <= 256 && !(elem_bytes & 3))) return PHX_OK;
  return fail(PHX_EINVAL, "%s: plane %d: elem_bytes = %d must be 1 or 4 * w with 1 <= w <= 64", fn, k, elem_bytes);
}
inline int frag_plane_src(const char* fn, const int k, const void* src, const int elem_bytes) {
  return elem_bytes != 1 && ((uintptr_t)src & 3u) ? fail(PHX_EINVAL, "%s: plane %d: src must be 4-byte aligned", fn, k) : PHX_OK;
}

// ---- phx_train_batch and phx_seq_batch --------------------------------------------------------------------------------------------
// phx_seq_batch_io repeats phx_train_batch_io's leading fields under the same names (`start` is `seq_start` there: passed in).  The
// rules the two calls share, in four runs: phx_seq_batch has rules of its own between them, and the order of the checks is kept.
template <typename IO>
int frag_batch_shape(const char* fn, const IO& io, const int tile_cols) {
  if (const int rc = frag_rows_cols(fn, io.T, io.N)) return rc;
  if (io.T > 0x7fffffffLL) return fail(PHX_EINVAL, "%s: T = %lld must be <= 2^31 - 1", fn, (long long)io.T);
  if (io.N > (1LL << 62) / io.T) return fail(PHX_EINVAL, "%s: T * N = %lld * %lld must be <= 2^62", fn, (long long)io.T, (long long)io.N);
  if (const int rc = frag_one_grid(fn, "N", io.N, tile_cols)) return rc;
  if (io.S < 1 || io.N % io.S != 0) return fail(PHX_EINVAL, "%s: S = %d must be >= 1 and divide N = %lld", fn, io.S, (long long)io.N);
  return PHX_OK;
}
template <typename IO>
int frag_batch_record(const char* fn, const IO& io, const int most_planes) {
  if (const int rc = frag_n_planes(fn, io.n_planes, most_planes)) return rc;
  if (const int rc = frag_row_words(fn, io.row_words)) return rc;
  return frag_at_least(fn, "capacity", io.capacity, 0);
}
template <typename IO>
int frag_batch_buffers(const char* fn, const IO& io, const void* start, const char* start_name) {
  if (io.shuffle != 0 && io.shuffle != 1) return fail(PHX_EINVAL, "%s: shuffle = %d must be 0 or 1", fn, io.shuffle);
  if (const int rc = frag_reserved(fn, io.reserved)) return rc;
  if (!start) return fail(PHX_EINVAL, "%s: %s is required", fn, start_name);
  if (io.n_planes > 0 && io.capacity > 0 && !io.records) return fail(PHX_EINVAL, "%s: records is required with n_planes > 0", fn);
  return PHX_OK;
}
// every plane inside the record and beside the others, then the standardized plane and its buffers
template <typename IO>
int frag_batch_planes(const char* fn, const IO& io) {
  bool used[256] = {};
  for (int k = 0; k < io.n_planes; ++k) {
    const auto& p = io.plane[k];
    if (!p.src) return fail(PHX_EINVAL, "%s: plane %d needs src", fn, k);
    if (const int rc = frag_plane_elem(fn, k, p.elem_bytes)) return rc;
    if (const int rc = frag_plane_src(fn, k, p.src, p.elem_bytes)) return rc;
    const int w = p.elem_bytes == 1 ? 1 : p.elem_bytes >> 2;
    if (p.word_off < 0 || p.word_off > io.row_words - w)
      return fail(PHX_EINVAL, "%s: plane %d: words [%d, %lld) lie outside the record of %d", fn, k, p.word_off, (long long)p.word_off + w,
                  io.row_words);
    for (int j = p.word_off; j < p.word_off + w; ++j) {
      if (used[j]) return fail(PHX_EINVAL, "%s: plane %d overlaps another plane at word %d", fn, k, j);
      used[j] = true;
    }
  }
  if (io.std_plane < -1 || io.std_plane >= io.n_planes)
    return fail(PHX_EINVAL, "%s: std_plane = %d must be -1 or a plane index below %d", fn, io.std_plane, io.n_planes);
  if (io.std_plane < 0) return PHX_OK;
  if (io.plane[io.std_plane].elem_bytes != 4) return fail(PHX_EINVAL, "%s: std_plane = %d must name a plane with elem_bytes 4", fn, io.std_plane);
  if (!io.moments || !io.workspace) return fail(PHX_EINVAL, "%s: std_plane needs moments and workspace", fn);
  return PHX_OK;
}

// the six round keys of the shuffle (include/phantom_amd_batch.h), for BtKeys / SqKeys
inline void frag_round_keys(const uint64_t seed, const uint64_t epoch, uint32_t (&key)[6]) {
  uint64_t s = seed ^ (epoch * 0x9E3779B97F4A7C15ull);
  for (int r = 0; r < 6; ++r) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    key[r] = (uint32_t)z;
  }
}
