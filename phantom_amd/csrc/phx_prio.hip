// phx_prio.hip -- phx_prio_add, phx_prio_update and phx_prio_sample (include/phantom_amd_prio.h): a 16-ary sum tree and min tree over
// the slots of a replay ring, kept on the device.  Nothing is read on the host; the kernels of a call are ordered by the
// stream alone.
//
// A node's 16 children are 64 contiguous, 64-byte aligned bytes: four dwordx4 loads issued together, then the chain of 15 adds in
// registers in the header's order (the build has -ffp-contract=off and no fast-math: the compiler keeps the order).
//   * A node is always RECOMPUTED from its children, sum and min alike; no delta is ever applied, so nothing drifts and threads that
//     share an ancestor store the same bits.
//   * Levels of more than PR_TOP nodes are "sparse": one launch per level touches only the ancestors of the slots a call names.
//     phx_prio_path_kernel (update) gives entry i the ancestor of slot_in[i].  phx_prio_span_kernel (add) knows that the named slots
//     are at most two contiguous runs, [base, min(base + cnt, C)) and [0, base + cnt - C), whose ancestors at a level are two runs of
//     nodes as well: thread t takes the t-th of them, so a run of 737 280 records costs 46 081 + 2 881 + 181 node recomputations, each
//     node once (twice where the two runs meet in a node).
//   * The remaining levels, the first of at most PR_TOP nodes and all above it, are recomputed whole by the one workgroup of
//     phx_prio_top_kernel, level after level with a workgroup barrier between them (at most 4 096 values read per level).
//   * update: phx_prio_zero_kernel clears the named leaves, phx_prio_raise_kernel raises each to san(p) with an integer atomicMax on its
//     bit pattern (order-preserving for non-negative floats, so the result is the maximum whatever the order), one wave-reduced
//     atomicMax into max_priority and one wave-reduced add into `ignored` per wave.
//   * sample: one thread per draw, L dependent node reads, no LDS, no atomics: latency-bound by design; the upper levels stay in cache.
//   * the select comes before the address: a slot outside [0, size) never forms one; cursor is taken mod C, size clamped to [0, C], and
//     the descent clamps j to the level's nodes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/phantom_amd_prio.h"
#include "phx_spec.h"
#include "phx_frag.h"

constexpr int PR_THREADS = 256;      // a workgroup: four waves
constexpr int PR_LEVELS = 9;         // levels 0 .. L, L <= 8 for C <= 2^30
constexpr int PR_TOP = 256;          // the top kernel recomputes the levels of at most this many nodes

typedef float pr_f32x4 __attribute__((ext_vector_type(4)));

// the header's n_l and off_l; min level l starts at min_base + off[l]; top: the first level >= 1 of at most PR_TOP nodes
struct PrLayout {
  int64_t n[PR_LEVELS], off[PR_LEVELS];
  int64_t min_base;
  int32_t L, top;
};

// one level l >= 1 of a launch: where its nodes and their children start (sum and min; min_child == off_child at level 1)
struct PrLevel {
  int64_t off_child, off_node, min_child, min_node;
  int32_t shift, leaves;             // slot >> shift is the slot's ancestor; leaves: l == 1
};

__device__ __forceinline__ int64_t pr_clamp_size(const int64_t size, const int64_t C) { return size < 0 ? 0 : size > C ? C : size; }

__device__ __forceinline__ int64_t pr_wrap_cursor(const int64_t cursor, const int64_t C) {
  const int64_t m = cursor % C;
  return m < 0 ? m + C : m;
}

__host__ __device__ __forceinline__ uint64_t pr_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float pr_san(const float p) { return p >= PHX_PRIO_MIN ? fminf(p, PHX_PRIO_MAX) : PHX_PRIO_MIN; }

__device__ __forceinline__ void pr_load16(const float* p, float c[16]) {
  const pr_f32x4* q = reinterpret_cast<const pr_f32x4*>(p);
  const pr_f32x4 a = q[0], b = q[1], d = q[2], e = q[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k] = a[k];
    c[4 + k] = b[k];
    c[8 + k] = d[k];
    c[12 + k] = e[k];
  }
}

// node j of a level from its 16 children: the sum chain and the minimum over the non-zero ones
__device__ __forceinline__ void pr_node(float* __restrict__ tree, const int64_t off_child, const int64_t off_node, const int64_t min_child,
                                        const int64_t min_node, const bool leaves, const int64_t j) {
  float c[16], v[16];
  pr_load16(tree + off_child + 16 * j, c);
  if (!leaves) pr_load16(tree + min_child + 16 * j, v);
  float s = c[0], mn = 0.0f;
#pragma unroll
  for (int k = 1; k < 16; ++k) s = s + c[k];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float x = leaves ? c[k] : v[k];
    mn = x > 0.0f && (mn == 0.0f || x < mn) ? x : mn;
  }
  tree[off_node + j] = s;
  tree[min_node + j] = mn;
}

// ---- add ------------------------------------------------------------------------------------------------------------------------
// the named slots as the header states them: cnt of them from `base` on, wrapping; false where the count is refused
__device__ __forceinline__ bool pr_add_span(const int64_t* __restrict__ ring_state, const int64_t* __restrict__ count_ptr, const int64_t count,
                                            const int64_t src_capacity, const int64_t C, int64_t& base, int64_t& cnt) {
  const int64_t K = count_ptr ? *count_ptr : count;
  if (K < 0 || K > src_capacity) return false;
  const int64_t j0 = K > C ? K - C : 0;
  base = pr_wrap_cursor(ring_state[0], C) + j0 % C;
  base = base >= C ? base - C : base;
  cnt = K - j0;                                                            // <= C
  return true;
}

__global__ __launch_bounds__(PR_THREADS) void phx_prio_fill_kernel(float* __restrict__ tree, phx_prio_state* __restrict__ state,
                                                                   const int64_t* __restrict__ ring_state, const int64_t* __restrict__ count_ptr,
                                                                   const int64_t count, const int64_t src_capacity, const int64_t C) {
  const int64_t t = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int64_t base, cnt;
  if (!pr_add_span(ring_state, count_ptr, count, src_capacity, C, base, cnt)) {
    if (t == 0) state->refused += 1;
    return;
  }
  if (t >= cnt) return;
  const float stored = state->max_priority;
  int64_t slot = base + t;                                                 // (base < C and t < cnt <= C)
  slot = slot >= C ? slot - C : slot;
  tree[slot] = stored == 0.0f ? 1.0f : stored;
}

__global__ __launch_bounds__(PR_THREADS) void phx_prio_span_kernel(float* __restrict__ tree, const int64_t* __restrict__ ring_state,
                                                                   const int64_t* __restrict__ count_ptr, const int64_t count,
                                                                   const int64_t src_capacity, const int64_t C, const PrLevel lv) {
  const int64_t t = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int64_t base, cnt;
  if (!pr_add_span(ring_state, count_ptr, count, src_capacity, C, base, cnt) || cnt == 0) return;
  const int64_t end = base + cnt;                                          // (<= 2 C - 1)
  const int64_t last1 = (end < C ? end : C) - 1;                           // the first run is [base, last1], never empty
  const int64_t n2 = end > C ? end - C : 0;                                // the second is [0, n2)
  const int64_t a1 = base >> lv.shift;
  const int64_t m1 = (last1 >> lv.shift) - a1 + 1;
  const int64_t m2 = n2 > 0 ? ((n2 - 1) >> lv.shift) + 1 : 0;
  if (t >= m1 + m2) return;
  pr_node(tree, lv.off_child, lv.off_node, lv.min_child, lv.min_node, lv.leaves != 0, t < m1 ? a1 + t : t - m1);
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void phx_prio_zero_kernel(float* __restrict__ tree, const int64_t* __restrict__ ring_state,
                                                                   const int64_t* __restrict__ slot_in, const int64_t n, const int64_t C) {
  const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t size = pr_clamp_size(ring_state[1], C);
  const int64_t slot = slot_in[i];
  if (slot >= 0 && slot < size) tree[slot] = 0.0f;
}

__global__ __launch_bounds__(PR_THREADS) void phx_prio_raise_kernel(float* __restrict__ tree, phx_prio_state* __restrict__ state,
                                                                    const int64_t* __restrict__ ring_state, const int64_t* __restrict__ slot_in,
                                                                    const float* __restrict__ priority, const int64_t n, const int64_t C) {
  const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  const int64_t size = pr_clamp_size(ring_state[1], C);
  const bool mine = i < n;
  const int64_t slot = mine ? slot_in[i] : -1;
  const bool valid = slot >= 0 && slot < size;
  const float p = pr_san(mine ? priority[i] : 0.0f);
  if (valid) atomicMax(reinterpret_cast<unsigned int*>(tree + slot), __float_as_uint(p));
  float top = valid ? fmaxf(p, 1.0f) : 0.0f;                               // (a stored 0 reads as 1: what is stored is at least 1)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = fmaxf(top, __shfl_xor(top, o));
  const unsigned long long out = __ballot(mine && !valid);
  if ((threadIdx.x & 63) == 0) {
    if (top > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&state->max_priority), __float_as_uint(top));
    if (out) atomicAdd(reinterpret_cast<unsigned long long*>(&state->ignored), (unsigned long long)__popcll(out));
  }
}

__global__ __launch_bounds__(PR_THREADS) void phx_prio_path_kernel(float* __restrict__ tree, const int64_t* __restrict__ ring_state,
                                                                   const int64_t* __restrict__ slot_in, const int64_t n, const int64_t C,
                                                                   const PrLevel lv) {
  const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t size = pr_clamp_size(ring_state[1], C);
  const int64_t slot = slot_in[i];
  if (slot < 0 || slot >= size) return;
  pr_node(tree, lv.off_child, lv.off_node, lv.min_child, lv.min_node, lv.leaves != 0, slot >> lv.shift);
}

// ---- both: the levels of at most PR_TOP nodes, whole, by one workgroup ------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void phx_prio_top_kernel(float* __restrict__ tree, const PrLayout ly) {
  for (int l = ly.top; l <= ly.L; ++l) {
    const int64_t j = threadIdx.x;
    if (j < ly.n[l])
      pr_node(tree, ly.off[l - 1], ly.off[l], ly.min_base + ly.off[l - 1], ly.min_base + ly.off[l], l == 1, j);
    __syncthreads();                                                       // (level l + 1 reads what this level stored)
  }
}

// ---- sample ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void phx_prio_sample_kernel(const float* __restrict__ tree, const int64_t* __restrict__ ring_state,
                                                                     int64_t* __restrict__ out_slot, float* __restrict__ out_priority,
                                                                     const int64_t n, const int64_t C, const uint64_t s0, const PrLayout ly) {
  const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t size = pr_clamp_size(ring_state[1], C);
  const float total = tree[ly.off[ly.L]];
  int64_t slot = -1;
  float leaf = 0.0f;
  if (total > 0.0f && size > 0) {
    const uint64_t x = pr_mix(s0 + ((uint64_t)i + 1ull) * 0x9E3779B97F4A7C15ull);
    float m = (float)(uint32_t)(x >> 40) * 0x1p-24f * total;
    int64_t j = 0;
    for (int l = ly.L; l >= 1; --l) {
      float c[16];
      pr_load16(tree + ly.off[l - 1] + 16 * j, c);
      float s = 0.0f, base = 0.0f, last_base = 0.0f;
      int ks = -1, last = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float prev = s;
        s = k == 0 ? c[0] : prev + c[k];
        const bool hit = ks < 0 && m < s;
        ks = hit ? k : ks;
        base = hit ? prev : base;
        last = c[k] > 0.0f ? k : last;
        last_base = c[k] > 0.0f ? prev : last_base;
      }
      base = ks < 0 ? last_base : base;
      ks = ks < 0 ? last : ks;
      m = m - base;
      j = 16 * j + ks;
      j = j < ly.n[l - 1] ? j : ly.n[l - 1] - 1;
    }
    const float v = tree[j];
    if (j < size && v > 0.0f) {
      slot = j;
      leaf = v;
    }
  }
  out_slot[i] = slot;
  out_priority[i] = leaf;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static PrLayout pr_layout(const int64_t C) {
  PrLayout ly = {};
  int l = 0;
  ly.n[0] = C;
  while (ly.n[l] != 1) {
    const int64_t w = 16 * ((ly.n[l] + 15) / 16);
    ly.off[l + 1] = ly.off[l] + w;
    ly.n[l + 1] = w / 16;
    ++l;
  }
  ly.L = l;
  ly.min_base = ly.off[l] + 16 - 16 * ((C + 15) / 16);                     // W - w_0
  ly.top = 1;
  while (ly.top <= ly.L && ly.n[ly.top] > PR_TOP) ++ly.top;
  return ly;
}

static PrLevel pr_level(const PrLayout& ly, const int l) {
  PrLevel lv;
  lv.off_child = ly.off[l - 1];
  lv.off_node = ly.off[l];
  lv.min_child = l == 1 ? ly.off[0] : ly.min_base + ly.off[l - 1];
  lv.min_node = ly.min_base + ly.off[l];
  lv.shift = 4 * l;
  lv.leaves = l == 1;
  return lv;
}

static unsigned pr_blocks(const int64_t threads) { return (unsigned)(threads < 1 ? 1 : (threads + PR_THREADS - 1) / PR_THREADS); }

static int pr_top(FragCall& call, float* tree, const PrLayout& ly, const hipStream_t st) {
  hipLaunchKernelGGL(phx_prio_top_kernel, dim3(1), dim3(PR_THREADS), 0, st, tree, ly);
  return call.launched("the top levels", "phx_prio_top_kernel");
}

// the three calls' capacity rule
static int pr_capacity(const char* fn, const int64_t capacity) {
  if (capacity < 1 || capacity > PHX_PRIO_MAX_CAPACITY) return fail(PHX_EINVAL, "%s: capacity = %lld must lie in [1, 2^30]", fn, (long long)capacity);
  return PHX_OK;
}

extern "C" int phx_prio_add(const phx_prio_add_io* io, void* stream) {
  const char* fn = "phx_prio_add";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = pr_capacity(fn, io->capacity)) return rc;
  if (const int rc = frag_at_least(fn, "src_capacity", io->src_capacity, 0)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved)) return rc;
  if (const int rc = frag_count(fn, io->count_ptr, io->count, io->src_capacity)) return rc;
  if (const int rc = frag_required(fn, io->ring_state && io->tree && io->state, "ring_state, tree and state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->tree, io->state), 16, "tree and state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->count_ptr, io->ring_state), 8, "count_ptr and ring_state")) return rc;
  const int64_t C = io->capacity;
  const int64_t most = io->src_capacity < C ? io->src_capacity : C;        // the host does not know K: the grids are sized from this
  const PrLayout ly = pr_layout(C);
  const hipStream_t st = (hipStream_t)stream;
  FragCall call{fn};
  hipLaunchKernelGGL(phx_prio_fill_kernel, dim3(pr_blocks(most)), dim3(PR_THREADS), 0, st, io->tree, io->state, io->ring_state, io->count_ptr,
                     io->count, io->src_capacity, C);
  if (const int rc = call.launched("the fill", "phx_prio_fill_kernel")) return rc;
  for (int l = 1; l < ly.top; ++l) {                                       // two runs of `most` slots in all: at most most / 16^l + 3 nodes
    hipLaunchKernelGGL(phx_prio_span_kernel, dim3(pr_blocks((most >> (4 * l)) + 3)), dim3(PR_THREADS), 0, st, io->tree, io->ring_state,
                       io->count_ptr, io->count, io->src_capacity, C, pr_level(ly, l));
    if (const int rc = call.launched("a sparse level", "phx_prio_span_kernel")) return rc;
  }
  return pr_top(call, io->tree, ly, st);
}

extern "C" int phx_prio_update(const phx_prio_update_io* io, void* stream) {
  const char* fn = "phx_prio_update";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = pr_capacity(fn, io->capacity)) return rc;
  if (const int rc = frag_at_least(fn, "n", io->n, 1)) return rc;
  if (const int rc = frag_one_grid(fn, "n", io->n, PR_THREADS)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved)) return rc;
  if (const int rc = frag_required(fn, io->slot_in && io->priority && io->ring_state && io->tree && io->state,
                                   "slot_in, priority, ring_state, tree and state"))
    return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->tree, io->state), 16, "tree and state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->slot_in, io->ring_state), 8, "slot_in and ring_state")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->priority), 4, "priority")) return rc;
  const int64_t C = io->capacity;
  const PrLayout ly = pr_layout(C);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(pr_blocks(io->n)), block(PR_THREADS);
  FragCall call{fn};
  hipLaunchKernelGGL(phx_prio_zero_kernel, grid, block, 0, st, io->tree, io->ring_state, io->slot_in, io->n, C);
  if (const int rc = call.launched("the zero fill", "phx_prio_zero_kernel")) return rc;
  hipLaunchKernelGGL(phx_prio_raise_kernel, grid, block, 0, st, io->tree, io->state, io->ring_state, io->slot_in, io->priority, io->n, C);
  if (const int rc = call.launched("the raise", "phx_prio_raise_kernel")) return rc;
  for (int l = 1; l < ly.top; ++l) {
    hipLaunchKernelGGL(phx_prio_path_kernel, grid, block, 0, st, io->tree, io->ring_state, io->slot_in, io->n, C, pr_level(ly, l));
    if (const int rc = call.launched("a sparse level", "phx_prio_path_kernel")) return rc;
  }
  return pr_top(call, io->tree, ly, st);
}

extern "C" int phx_prio_sample(const phx_prio_sample_io* io, void* stream) {
  const char* fn = "phx_prio_sample";
  if (const int rc = frag_io(fn, io)) return rc;
  if (const int rc = pr_capacity(fn, io->capacity)) return rc;
  if (const int rc = frag_at_least(fn, "n", io->n, 1)) return rc;
  if (const int rc = frag_one_grid(fn, "n", io->n, PR_THREADS)) return rc;
  if (const int rc = frag_reserved(fn, io->reserved)) return rc;
  if (const int rc = frag_required(fn, io->ring_state && io->tree && io->out_slot && io->out_priority, "ring_state, tree, out_slot and out_priority"))
    return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->tree, io->out_slot, io->out_priority), 16, "tree, out_slot and out_priority")) return rc;
  if (const int rc = frag_aligned(fn, frag_bits(io->ring_state), 8, "ring_state")) return rc;
  const uint64_t s0 = pr_mix(pr_mix(io->seed + 0x9E3779B97F4A7C15ull) ^ io->draw);
  hipLaunchKernelGGL(phx_prio_sample_kernel, dim3(pr_blocks(io->n)), dim3(PR_THREADS), 0, (hipStream_t)stream, io->tree, io->ring_state,
                     io->out_slot, io->out_priority, io->n, io->capacity, s0, pr_layout(io->capacity));
  return FragCall{fn}.launched("the draw", "phx_prio_sample_kernel");
}
