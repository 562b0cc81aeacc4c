// phx_replay.hip -- phx_replay_add and phx_replay_sample (include/phantom_amd_replay.h): a ring of records on the device, appended to
// with the count read from device memory and sampled uniformly.  Two copy-shaped kernels and a one-thread commit; no
// atomics, no LDS, nothing read on the host.
//
// The unit of work is one 16-byte PIECE of a record: a record is P = row_words / 4 consecutive lanes, every load and store a whole
// dwordx4.  A workgroup of 256 threads owns a TILE of R = floor(1024 / P) consecutive records, RP_U = 4 pieces per lane: piece
// l = u * 256 + thread of the tile belongs to the tile's record l / P (a multiply by the host's 2^32 / P rounded up: l < 1024, exact
// below 2^26) -- no 64-bit division per piece, and the lanes beyond R * P (P does not divide 1024) sit out.
//   * consecutive lanes cover consecutive pieces of consecutive records: the add's loads from `src` and the sample's stores to `out`
//     are one contiguous run per wave-instruction; the ring's side of each copy moves in whole-record runs of 16 * P bytes;
//   * a lane's RP_U loads are issued before its first store, so a wave has RP_U * 64 / P records in flight (64 for a 64-byte record):
//     a single dependent read would pay the whole miss.  With slot_in the RP_U slot loads go first, then the RP_U ring loads;
//   * the select comes before the load: a slot outside [0, size) reads slot 0 (the ring has C >= 1 slots) and its words are replaced
//     by zeros, so nothing the caller or a broken state supplies becomes an address; cursor is taken mod C and size clamped to [0, C];
//   * phx_replay_add_kernel walks its tiles in a grid-stride loop from record max(0, K - C) and leaves it at K, both read on the
//     device; the state is written by phx_replay_commit_kernel alone, one thread, after every read of the old one (stream order);
//   * the ring is written with non-temporal stores (it is read again much later, at random) and `out` with plain ones (the learner
//     reads it next): DESIGN 3.4n has the numbers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_replay.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int RP_THREADS = 256;      // a workgroup: four waves
constexpr int RP_U = 4;              // pieces per lane and tile: loads in flight per lane
constexpr int RP_TILE = RP_THREADS * RP_U;      // pieces per tile
constexpr int RP_MAX_GRID = 8192;    // workgroups of the add's grid-stride loop: 32 per CU

typedef uint32_t rp_u32x4 __attribute__((ext_vector_type(4)));

// what the host derives from row_words once: P, R = RP_TILE / P and ceil(2^32 / P)
struct RpShape {
  uint32_t P, R;
  uint64_t magic;
};

__device__ __forceinline__ int64_t rp_clamp_size(const int64_t size, const int64_t C) { return size < 0 ? 0 : size > C ? C : size; }

__device__ __forceinline__ int64_t rp_wrap_cursor(const int64_t cursor, const int64_t C) {
  const int64_t m = cursor % C;
  return m < 0 ? m + C : m;
}

__host__ __device__ __forceinline__ uint64_t rp_mix(uint64_t z) {      // (the host mixes seed and draw into s0 once per call)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(RP_THREADS) void phx_replay_add_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ ring,
                                                                    const phx_replay_state* __restrict__ state,
                                                                    const int64_t* __restrict__ count_ptr, const int64_t count,
                                                                    const int64_t src_capacity, const int64_t C, const RpShape sh) {
  const int64_t K = count_ptr ? *count_ptr : count;
  if (K < 0 || K > src_capacity) return;                                   // (refused: every lane of the grid alike)
  const int64_t j0 = K > C ? K - C : 0;                                    // the first record that is kept
  uint64_t base = (uint64_t)rp_wrap_cursor(state->cursor, C) + (uint64_t)(j0 % C);      // the slot of record j0
  base = base >= (uint64_t)C ? base - (uint64_t)C : base;
  uint32_t r[RP_U], k[RP_U];
#pragma unroll
  for (int u = 0; u < RP_U; ++u) {
    const uint32_t l = (uint32_t)(u * RP_THREADS) + threadIdx.x;
    r[u] = (uint32_t)((l * sh.magic) >> 32);
    k[u] = l - r[u] * sh.P;
  }
  for (int64_t j = j0 + (int64_t)blockIdx.x * sh.R; j < K; j += (int64_t)gridDim.x * sh.R) {
    rp_u32x4 v[RP_U];
#pragma unroll
    for (int u = 0; u < RP_U; ++u) {
      const int64_t jr = j + r[u];
      const int64_t jc = r[u] < sh.R && jr < K ? jr : K - 1;              // (past the tile or the count: the last record again, dropped)
      v[u] = *reinterpret_cast<const rp_u32x4*>(src + ((jc * sh.P + k[u]) << 2));
    }
#pragma unroll
    for (int u = 0; u < RP_U; ++u) {
      const int64_t jr = j + r[u];
      if (r[u] < sh.R && jr < K) {
        uint64_t slot = base + (uint64_t)(jr - j0);                        // (jr - j0 < C and base < C)
        slot = slot >= (uint64_t)C ? slot - (uint64_t)C : slot;
        __builtin_nontemporal_store(v[u], reinterpret_cast<rp_u32x4*>(ring + (((int64_t)slot * sh.P + k[u]) << 2)));
      }
    }
  }
}

__global__ __launch_bounds__(64) void phx_replay_commit_kernel(phx_replay_state* __restrict__ state, const int64_t* __restrict__ count_ptr,
                                                               const int64_t count, const int64_t src_capacity, const int64_t C) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t K = count_ptr ? *count_ptr : count;
  phx_replay_state s = *state;
  if (K < 0 || K > src_capacity) {
    s.refused += 1;
  } else {
    const uint64_t c = (uint64_t)rp_wrap_cursor(s.cursor, C) + (uint64_t)(K % C);
    const int64_t size = rp_clamp_size(s.size, C);
    s.cursor = (int64_t)(c >= (uint64_t)C ? c - (uint64_t)C : c);
    s.size = K >= C - size ? C : size + K;
    s.total += K;
  }
  *state = s;
}

__global__ __launch_bounds__(RP_THREADS) void phx_replay_sample_kernel(const uint32_t* __restrict__ ring, const phx_replay_state* __restrict__ state,
                                                                       const int64_t* __restrict__ slot_in, uint32_t* __restrict__ out,
                                                                       int64_t* __restrict__ out_slot, const int64_t n, const int64_t C,
                                                                       const uint64_t s0, const RpShape sh) {
  const int64_t size = rp_clamp_size(state->size, C);
  const int64_t i0 = (int64_t)blockIdx.x * sh.R;                           // the tile's first record
  int64_t i[RP_U], s[RP_U];
  uint32_t k[RP_U];
  bool mine[RP_U];
#pragma unroll
  for (int u = 0; u < RP_U; ++u) {
    const uint32_t l = (uint32_t)(u * RP_THREADS) + threadIdx.x;
    const uint32_t r = (uint32_t)((l * sh.magic) >> 32);
    k[u] = l - r * sh.P;
    mine[u] = r < sh.R && i0 + r < n;
    i[u] = mine[u] ? i0 + r : n - 1;                                       // (past the tile or n: the last record again, dropped)
  }
  if (slot_in) {                                                           // (uniform)
#pragma unroll
    for (int u = 0; u < RP_U; ++u) s[u] = slot_in[i[u]];
#pragma unroll
    for (int u = 0; u < RP_U; ++u) s[u] = s[u] >= 0 && s[u] < size ? s[u] : -1;
  } else {
#pragma unroll
    for (int u = 0; u < RP_U; ++u) {
      const uint64_t x = rp_mix(s0 + ((uint64_t)i[u] + 1ull) * 0x9E3779B97F4A7C15ull);
      s[u] = size > 0 ? (int64_t)__umul64hi(x, (uint64_t)size) : -1;
    }
  }
  rp_u32x4 v[RP_U];
#pragma unroll
  for (int u = 0; u < RP_U; ++u) {
    const int64_t sc = s[u] >= 0 ? s[u] : 0;                               // the select before the load
    v[u] = *reinterpret_cast<const rp_u32x4*>(ring + ((sc * sh.P + k[u]) << 2));
  }
#pragma unroll
  for (int u = 0; u < RP_U; ++u) {
    if (mine[u]) {
      const rp_u32x4 zero = {0u, 0u, 0u, 0u};
      *reinterpret_cast<rp_u32x4*>(out + ((i[u] * sh.P + k[u]) << 2)) = s[u] >= 0 ? v[u] : zero;
      if (out_slot && k[u] == 0) out_slot[i[u]] = s[u];
    }
  }
}

static RpShape rp_shape(const int row_words) {
  RpShape sh;
  sh.P = (uint32_t)row_words >> 2;
  sh.R = (uint32_t)RP_TILE / sh.P;
  sh.magic = ((1ull << 32) + sh.P - 1) / sh.P;
  return sh;
}

// the tiles of `records` records (sh.R a tile: what frag_one_grid is given)
static int64_t rp_tiles(const int64_t records, const RpShape& sh) { return records / sh.R + (records % sh.R ? 1 : 0); }

extern "C" int phx_replay_add(const phx_replay_add_io* io, void* stream) {
  const char* fn = "phx_replay_add";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_at_least(fn, "capacity", io->capacity, 1)) return rc;
  if (const int rc = frag_at_least(fn, "src_capacity", io->src_capacity, 0)) return rc;
  if (const int rc = frag_row_words(fn, io->row_words)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved, io->reserved0)) return rc;
  if (const int rc = frag_count(fn, io->count_ptr, io->count, io->src_capacity)) return rc;
  if (const int rc = frag_required(fn, io->ring && io->state, "ring and state")) return rc;
  if (io->src_capacity > 0 && !io->src) return fail(PHX_EINVAL, "phx_replay_add: src is required with src_capacity > 0");
  if (const int rc = frag_aligned(fn, frag_bits(io->src, io->ring, io->state), 16, "src, ring and state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->count_ptr), 8, "count_ptr")) return rc;
  const RpShape sh = rp_shape(io->row_words);
  if (const int rc = frag_one_grid(fn, "src_capacity", io->src_capacity, sh.R)) return rc;
  const int64_t tiles = rp_tiles(io->src_capacity, sh);
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  const unsigned grid = (unsigned)(tiles < 1 ? 1 : tiles < RP_MAX_GRID ? tiles : RP_MAX_GRID);      // (src_capacity == 0: K == 0, nothing is read)
  hipLaunchKernelGGL(phx_replay_add_kernel, dim3(grid), dim3(RP_THREADS), 0, st, io->src, io->ring, io->state, io->count_ptr, io->count,
                     io->src_capacity, io->capacity, sh);
  if (const int rc = call.launched("the copy", "phx_replay_add_kernel")) return rc;
  hipLaunchKernelGGL(phx_replay_commit_kernel, dim3(1), dim3(64), 0, st, io->state, io->count_ptr, io->count, io->src_capacity, io->capacity);
  return call.launched("the commit", "phx_replay_commit_kernel");
}

extern "C" int phx_replay_sample(const phx_replay_sample_io* io, void* stream) {
  const char* fn = "phx_replay_sample";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = frag_at_least(fn, "capacity", io->capacity, 1)) return rc;
  if (const int rc = frag_at_least(fn, "n", io->n, 1)) return rc;
  if (const int rc = frag_row_words(fn, io->row_words)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved, io->reserved0)) return rc;
  if (const int rc = frag_required(fn, io->ring && io->state && io->out, "ring, state and out")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->ring, io->state, io->out, io->out_slot), 16, "ring, state, out and out_slot")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->slot_in), 8, "slot_in")) return rc;
  const RpShape sh = rp_shape(io->row_words);
  if (const int rc = frag_one_grid(fn, "n", io->n, sh.R)) return rc;
  const uint64_t s0 = rp_mix(rp_mix(io->seed + 0x9E3779B97F4A7C15ull) ^ io->draw);
  hipLaunchKernelGGL(phx_replay_sample_kernel, dim3((unsigned)rp_tiles(io->n, sh)), dim3(RP_THREADS), 0, (hipStream_t)stream, io->ring, io->state,
                     io->slot_in, io->out, io->out_slot, io->n, io->capacity, s0, sh);
  return FragCall{fn}.launched(nullptr, "phx_replay_sample_kernel");
}
