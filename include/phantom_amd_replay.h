/*
 * phantom_amd_replay.h -- a replay learner's buffer on the device: a RING of records (the records of phantom_amd_batch.h: all columns
 * of a transition contiguous, a multiple of 16 bytes) that a batch's records are appended to with the count taken from device memory,
 * and that minibatches of records are drawn from uniformly -- DQN / SAC / TD3 / DDPG train on old transitions many times, and neither
 * call reads anything on the host.
 *
 * A tenth, additive header of libphantom_amd.so: nothing in the other nine changes (PHX_ABI_VERSION stays 10, the return codes and
 * phx_last_error / phx_last_kernel are the ones declared in phantom_amd.h).  Like the other additive headers the functions take no env
 * handle: buffers in, buffers out, on the current device, asynchronously on `stream`.
 *
 * Ring and state.  A ring is uint32_t ring[C][row_words], row_words a multiple of 4 in [4, 256] as in phantom_amd_batch.h, and comes
 * with a 32-byte device-resident phx_replay_state that only these kernels read and write.  All zero is the empty ring: the caller
 * zero-fills the state once (the ring itself needs no fill).  Invariant: while size < C, cursor == size -- which is why the valid slots
 * are always exactly [0, size).
 *
 * phx_replay_add, evaluated on the device in stream order:
 *
 *   K = count_ptr ? *count_ptr : count
 *   K < 0 or K > src_capacity:   refused += 1 and nothing else changes (a batch whose K exceeded its capacity holds no records:
 *                                "nothing was written" in phantom_amd_batch.h)
 *   otherwise, for every j with max(0, K - C) <= j < K:   record j of src is copied bit for bit to slot (cursor + j) mod C
 *                                (the last min(K, C) records, in order: no slot has two writers)
 *   then   cursor = (cursor + K) mod C,   size = min(C, size + K),   total += K
 *
 * No byte of `ring` outside the named slots is written.  The state is committed only after every read of the old state: the call is
 * two launches, phx_replay_add_kernel (its grid sized from src_capacity, the host does not know K) and the one-thread
 * phx_replay_commit_kernel; phx_last_kernel() then reads "phx_replay_add_kernel+phx_replay_commit_kernel".
 *
 * phx_replay_sample, with `size` read from the state on the device, for i = 0 .. n - 1:
 *
 *   with slot_in:      s_i = slot_in[i] if 0 <= slot_in[i] < size, else -1
 *   without slot_in:   s_i = -1 if size == 0; otherwise a uniform draw with replacement (RLlib's ReplayBuffer.sample), in integer
 *                      arithmetic mod 2^64:
 *
 *                        G = 0x9E3779B97F4A7C15
 *                        mix(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *                        s0  = mix(mix(seed + G) ^ draw)
 *                        u_i = mix(s0 + (i + 1) * G)
 *                        s_i = (u_i * size) >> 64              the high half of the 128-bit product
 *
 *   out[i] = ring[s_i] bit for bit (NaN payloads and -0.0 survive), or all zero words where s_i == -1;   out_slot[i] = s_i
 *
 * Every element of out and out_slot is written.  The select happens before the load: a slot_in value outside [0, size), INT64_MIN and
 * INT64_MAX included, never becomes an address.  phx_last_kernel() reads "phx_replay_sample_kernel".
 *
 * Both calls.  ring, src, out, out_slot and state are 16-byte aligned, count_ptr and slot_in 8-byte.  Element offsets are 64-bit.  src
 * and out must not overlap ring.  Calls on one ring must be on one stream, or ordered by the caller.  A state that zero-fill and these
 * calls did not produce gives undefined results; the kernels still clamp what they read from it, size to [0, C] and cursor mod C, so
 * they never index outside `ring`.
 *
 * Out of scope: prioritized sampling (slot_in / out_slot are its building block: phantom_amd_prio.h draws the slots), sampling without
 * replacement, sequence batches, spilling to the host, more than one GPU.
 * (tests/replay_ref.py, tests/test_replay_cpu.py, tests/test_gpu_replay.py)
 */
#ifndef PHANTOM_AMD_REPLAY_H
#define PHANTOM_AMD_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_replay_state {   /* on the device; all zero == an empty ring (the caller zero-fills it once) */
  int64_t cursor;                   /* 0    the slot the next record goes to, in [0, C)                         */
  int64_t size;                     /* 8    valid records: exactly the slots [0, size), size <= C               */
  int64_t total;                    /* 16   records ever accepted                                               */
  int64_t refused;                  /* 24   add calls whose count lay outside [0, src_capacity]                 */
} phx_replay_state;                 /* 32 bytes */

typedef struct phx_replay_add_io {
  int64_t capacity;                 /* 0    C, the ring's slots (>= 1)                                          */
  int64_t src_capacity;             /* 8    records that src holds (>= 0)                                       */
  int64_t count;                    /* 16   K, used when count_ptr is NULL: in [0, src_capacity]                */
  int32_t row_words;                /* 24   32-bit words per record: a multiple of 4 in [4, 256]                */
  int32_t reserved0;                /* 28   0                                                                   */
  const int64_t* count_ptr;         /* 32   K on the device, or NULL                                            */
  const uint32_t* src;              /* 40   [src_capacity][row_words]; required with src_capacity > 0           */
  uint32_t* ring;                   /* 48   [capacity][row_words] required                                      */
  phx_replay_state* state;          /* 56   required                                                            */
  int64_t reserved[2];              /* 64   0                                                                   */
} phx_replay_add_io;                /* 80 bytes */

typedef struct phx_replay_sample_io {
  int64_t capacity;                 /* 0    C, the ring's slots (>= 1)                                          */
  int64_t n;                        /* 8    records to draw (>= 1)                                              */
  int32_t row_words;                /* 16   32-bit words per record: a multiple of 4 in [4, 256]                */
  int32_t reserved0;                /* 20   0                                                                   */
  uint64_t seed;                    /* 24   seed and draw select the stream of draws (not read with slot_in)    */
  uint64_t draw;                    /* 32                                                                       */
  const int64_t* slot_in;           /* 40   [n], or NULL: the slots are drawn                                   */
  const uint32_t* ring;             /* 48   [capacity][row_words] required                                      */
  const phx_replay_state* state;    /* 56   required                                                            */
  uint32_t* out;                    /* 64   [n][row_words] required                                             */
  int64_t* out_slot;                /* 72   [n], or NULL                                                        */
  int64_t reserved[2];              /* 80   0                                                                   */
} phx_replay_sample_io;             /* 96 bytes */

/* Both return PHX_OK, or PHX_EINVAL with a phx_last_error text that names the function: io or a required pointer NULL; a misaligned
 * pointer; capacity < 1; src_capacity < 0, or n < 1; row_words not a multiple of 4 in [4, 256]; a host count outside [0, src_capacity]
 * when count_ptr is NULL; a non-zero reserved field; sizes beyond one launch's grid (more than 2^31 - 1 tiles of floor(1024 /
 * (row_words / 4)) records in src_capacity or n).  Nothing is launched then.  PHX_EHIP: a launch failed. */
int phx_replay_add(const phx_replay_add_io* io, void* stream);
int phx_replay_sample(const phx_replay_sample_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHANTOM_AMD_REPLAY_H */
