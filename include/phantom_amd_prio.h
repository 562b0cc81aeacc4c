/*
 * phantom_amd_prio.h -- prioritized replay on the device: a SUM TREE and a MIN TREE over the slots of the ring of
 * phantom_amd_replay.h, kept in one device buffer next to it.  Three calls fill it for added records, update it from TD errors and
 * draw slots proportionally to priority (RLlib's PrioritizedReplayBuffer, which DQN, Ape-X and optionally SAC use); the ring's own
 * sample call then gathers the drawn slots' records through its slot_in.  No call reads anything on the host.
 *
 * An eleventh, additive header of libphantom_amd.so: nothing in the other ten changes (PHX_ABI_VERSION stays 10, the return codes and
 * phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like the other additive headers the functions take no env
 * handle: buffers in, buffers out, on the current device, asynchronously on `stream`.  The ring's 32-byte state is passed as
 * const int64_t* ring_state (4 x i64: cursor, size, total, refused) and only read.
 *
 * Tree.  PHX_PRIO_FANOUT = 16.  For a ring of C slots, 1 <= C <= 2^30:
 *
 *   n_0 = C,   w_l = 16 * ceil(n_l / 16),   n_{l+1} = w_l / 16;   L is the first level with n_L == 1   (C == 1: L == 0; C == 2^30: L == 8)
 *   off_0 = 0,   off_{l+1} = off_l + w_l,   W = off_L + 16
 *
 * One buffer float tree[W + (W - w_0)] holds both trees: sum level l (0 .. L) at off_l, min level l (1 .. L) at W + off_l - w_0.  All
 * zero is the empty tree: the caller zero-fills the buffer once.  The padding (the w_l - n_l words behind a level) stays zero.  Leaf s
 * = sum[s] is the priority of ring slot s, 0 for a slot that holds no record or never got a priority.
 *
 * Invariant after every call, for every node j < n_l of every level l >= 1, with children c_k = sum[off_{l-1} + 16 j + k]:
 *
 *   s_0 = c_0,   s_k = s_{k-1} + c_k   (a sequential chain of f32 adds);   sum[off_l + j] == s_15 bit for bit
 *   min[l][j] = the minimum over the non-zero values among its 16 children -- the leaves c_k at level 1, min[l-1][16 j + k] above --
 *               or 0 if there are none  (no value is negative)
 *
 * total = sum[off_L] is the root of the sum tree; pmin, the root of the min tree, is min[L][0] (L == 0: the one leaf, tree[0]).  A call
 * may rewrite a node whose children did not change with the value it already holds; nothing else of the buffer is written.
 *
 * State.  phx_prio_state, 32 bytes on the device, zero-filled once.  A stored max_priority of 0 reads as 1.0f, RLlib's initial one.
 *
 * Sanitize.  PHX_PRIO_MIN = 2^-40, PHX_PRIO_MAX = 2^40;   san(p) = p >= PHX_PRIO_MIN ? min(p, PHX_PRIO_MAX) : PHX_PRIO_MIN.   NaN, zero and
 * negatives become PHX_PRIO_MIN and +inf PHX_PRIO_MAX: no sum overflows or is NaN, and a held record never has priority 0.
 *
 * phx_prio_add -- called BEFORE the ring's add of the same batch, on the same stream, with the same capacity, src_capacity, count,
 * count_ptr and the ring's state (not yet advanced):
 *
 *   K = count_ptr ? *count_ptr : count
 *   K < 0 or K > src_capacity:   state.refused += 1 and nothing else changes
 *   otherwise, for every j with max(0, K - C) <= j < K:   leaf (cursor + j) mod C = max_priority as read above (cursor taken mod C)
 *                                -- exactly the slots the ring's add will write -- and the invariant is restored
 *
 * phx_prio_update -- n >= 1 entries (slot_in[i], priority[i]); the caller passes priorities already raised to alpha:
 *
 *   an entry with slot_in[i] outside [0, size) is ignored and counted in state.ignored (size clamped to [0, C]; the select comes before
 *   any address is formed: INT64_MIN and INT64_MAX are harmless)
 *   every slot named by at least one accepted entry:   leaf = max over its accepted entries of san(priority[i])   (independent of the
 *                                order of execution; duplicates of a minibatch drawn with replacement carry the same TD error anyway)
 *   with at least one accepted entry:   max_priority = max(max_priority as read above, every accepted san(priority[i]))
 *   and the invariant is restored
 *
 * phx_prio_sample -- n >= 1 draws, out_slot[i] and out_priority[i] both written for every i; size clamped to [0, C]:
 *
 *   total == 0 or size == 0:   out_slot[i] = -1, out_priority[i] = +0.0
 *   otherwise, in integer arithmetic mod 2^64 (the stream of draws of phantom_amd_replay.h):
 *
 *     G = 0x9E3779B97F4A7C15
 *     mix(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *     s0  = mix(mix(seed + G) ^ draw),   x_i = mix(s0 + (i + 1) * G)
 *     u   = (float)(x_i >> 40) * 2^-24      (exact)
 *     m   = u * total                       (one f32 rounding: m < total)
 *
 *   then the descent from the root, j = 0: at each level l = L .. 1 read node j's 16 children c_k and form s_k as in the invariant;
 *
 *     k* = the first k with m < s_k;  if there is none (the f32 subtraction below can leave m slightly above the chosen child's own
 *          sum), the last k with c_k > 0;  if there is none either (a state these calls did not produce), 0
 *     m  = m - (k* > 0 ? s_{k*-1} : 0)
 *     j  = min(16 j + k*, n_{l-1} - 1)      (the clamp binds only in a state these calls did not produce; with it every index
 *                                            formed lies inside the buffer)
 *
 *   The rule reaches a leaf with priority > 0 whenever the invariant holds.  The final j is the slot: out_slot[i] = j and
 *   out_priority[i] = leaf j bit for bit -- or -1 and +0.0 if j >= size or the leaf is 0.
 *
 * Known answers (tests/test_prio_cpu.py): C = 37, size = 37, leaf s = 1 + s mod 7 through phx_prio_update; n = 8:
 *   (seed, draw) = (0, 0):            slots 12 11 11 18 22 17  4  8,   priorities 6 5 5 5 2 4 5 2
 *   (0, 1):                           slots 19 11 34  6 13 10  6  9,   priorities 6 5 7 7 7 4 7 3
 *   (1, 0):                           slots 16 16 20 30  6  5 27 13,   priorities 3 3 7 3 7 6 7 7
 *   (2^64 - 1, 2^64 - 1):             slots 26  1  0 33 18 18 25 31,   priorities 6 2 1 6 5 5 5 4
 *
 * Launches, in stream order (no grid-wide barrier; no kernel reads a state field that another kernel of the same call writes).
 * phx_last_kernel() reads the names joined by "+", a name once however often its kernel was launched:
 *   phx_prio_add:      "phx_prio_fill_kernel+phx_prio_span_kernel+phx_prio_top_kernel"
 *   phx_prio_update:   "phx_prio_zero_kernel+phx_prio_raise_kernel+phx_prio_path_kernel+phx_prio_top_kernel"
 *   phx_prio_sample:   "phx_prio_sample_kernel"
 * The span and path kernels run once per level of more than 256 nodes, so their names are missing for C <= 4096.
 *
 * All calls.  tree, state, out_slot and out_priority are 16-byte aligned, slot_in, count_ptr and ring_state 8-byte, priority 4-byte.
 * Calls on one tree must be on the ring's stream, or ordered by the caller.  A tree or state that zero-fill and these calls did not
 * produce gives undefined results, but no access outside the buffers.
 *
 * Out of scope: stratified draws, sampling without replacement, a slot overwritten by an add between its draw and its update (its new
 * record then gets the old record's priority; RLlib has the same hazard), more than one GPU.
 * (tests/prio_ref.py, tests/test_prio_cpu.py, tests/test_gpu_prio.py)
 */
#ifndef PHANTOM_AMD_PRIO_H
#define PHANTOM_AMD_PRIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_PRIO_FANOUT 16
#define PHX_PRIO_MIN 0x1p-40f
#define PHX_PRIO_MAX 0x1p+40f
#define PHX_PRIO_MAX_CAPACITY (1 << 30)

typedef struct phx_prio_state {     /* on the device; all zero == nothing happened yet (the caller zero-fills it once) */
  float max_priority;               /* 0    the largest priority ever accepted, at least 1; a stored 0 reads as 1.0f */
  uint32_t reserved0;               /* 4    0                                                                   */
  int64_t ignored;                  /* 8    update entries whose slot lay outside [0, size)                     */
  int64_t refused;                  /* 16   add calls whose count lay outside [0, src_capacity]                 */
  int64_t reserved1;                /* 24   0                                                                   */
} phx_prio_state;                   /* 32 bytes */

typedef struct phx_prio_add_io {
  int64_t capacity;                 /* 0    C, the ring's slots: in [1, 2^30]                                   */
  int64_t src_capacity;             /* 8    records the batch's buffer holds (>= 0)                             */
  int64_t count;                    /* 16   K, used when count_ptr is NULL: in [0, src_capacity]                */
  const int64_t* count_ptr;         /* 24   K on the device, or NULL                                            */
  const int64_t* ring_state;        /* 32   the ring's 32-byte state, BEFORE the ring's add; required           */
  float* tree;                      /* 40   [W + (W - w_0)] required                                            */
  phx_prio_state* state;            /* 48   required                                                            */
  int64_t reserved[2];              /* 56   0                                                                   */
} phx_prio_add_io;                  /* 72 bytes */

typedef struct phx_prio_update_io {
  int64_t capacity;                 /* 0    C, the ring's slots: in [1, 2^30]                                   */
  int64_t n;                        /* 8    entries (>= 1)                                                      */
  const int64_t* slot_in;           /* 16   [n] required                                                        */
  const float* priority;            /* 24   [n] required: already raised to alpha                               */
  const int64_t* ring_state;        /* 32   the ring's 32-byte state; required                                  */
  float* tree;                      /* 40   [W + (W - w_0)] required                                            */
  phx_prio_state* state;            /* 48   required                                                            */
  int64_t reserved[2];              /* 56   0                                                                   */
} phx_prio_update_io;               /* 72 bytes */

typedef struct phx_prio_sample_io {
  int64_t capacity;                 /* 0    C, the ring's slots: in [1, 2^30]                                   */
  int64_t n;                        /* 8    draws (>= 1)                                                        */
  uint64_t seed;                    /* 16   seed and draw select the stream of draws                            */
  uint64_t draw;                    /* 24                                                                       */
  const int64_t* ring_state;        /* 32   the ring's 32-byte state; required                                  */
  const float* tree;                /* 40   [W + (W - w_0)] required                                            */
  int64_t* out_slot;                /* 48   [n] required                                                        */
  float* out_priority;              /* 56   [n] required                                                        */
  int64_t reserved[2];              /* 64   0                                                                   */
} phx_prio_sample_io;               /* 80 bytes */

/* All return PHX_OK, or PHX_EINVAL with a phx_last_error text that names the function: io or a required pointer NULL; a misaligned
 * pointer; capacity outside [1, 2^30]; src_capacity < 0, or n < 1; a host count outside [0, src_capacity] when count_ptr is NULL; a
 * non-zero reserved field; sizes beyond one launch's grid (n above 256 * (2^31 - 1)).  Nothing is launched then.  PHX_EHIP: a launch
 * failed. */
int phx_prio_add(const phx_prio_add_io* io, void* stream);
int phx_prio_update(const phx_prio_update_io* io, void* stream);
int phx_prio_sample(const phx_prio_sample_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_PRIO_H */
