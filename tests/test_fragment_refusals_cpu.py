"""CPU: every refusal of the sixteen fragment entry points (include/phantom_amd_{gae,vtrace,traj,compact,nstep,episodes,batch,seq,
replay,prio,filter}.h), verbatim: the return code and the whole phx_last_error() text, for one accepted io struct per entry point and
one patch per case.  Every refusal returns before the first HIP call, so the built library answers here without a GPU.

The cases of an entry point stand in the order of its checks and reach each of its PHX_EINVAL sites, each clause of an OR-ed check
included (every pointer of an alignment group, NaN as well as out of range, every reserved word).  PAIRS breaks two rules that are
adjacent in the check order of phx_train_batch, phx_seq_batch, phx_replay_add and phx_prio_add at once: the earlier one must answer.
No site is unreachable.

The structs carry addresses that point nowhere: a case accepted by mistake must fail at its launch (PHX_EHIP without a GPU), never run,
so the module skips itself where a GPU is visible and every case looks at the return code first."""
import ctypes as C
import re

import pytest
import torch

from phantom_amd import _abi

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the io structs point nowhere: not to be launched on a GPU")

PHX_EINVAL = -1
OPS = {**_abi.FRAGMENT_OPS, **_abi.PRIORITY_OPS, **_abi.FILTER_OPS}
NAN, INF = float("nan"), float("inf")
GRID64 = 64 * 0x7fffffff + 1           # columns past a grid of 64-lane workgroups
GRID256 = 256 * 0x7fffffff + 1         # elements past a grid of 256-thread workgroups


def A(i):
    """a made-up device address, 16-byte aligned, far from every other one"""
    return 0x10000000 * (i + 1)


def ptrs(*names):
    return {n: A(i) for i, n in enumerate(names)}


BATCH_PLANES = {"plane[0].src": A(20), "plane[0].elem_bytes": 4, "plane[0].word_off": 0,
                "plane[1].src": A(21), "plane[1].elem_bytes": 1, "plane[1].word_off": 1}
BATCH = dict(T=4, N=8, capacity=16, n_planes=2, row_words=8, S=2, class_id=0, std_plane=0, shuffle=1, seed=1, epoch=0, **BATCH_PLANES)

# one io struct per entry point that passes every check
GOOD = {
    "phx_gae": dict(T=4, N=8, gamma=0.5, lambda_=0.25,
                    **ptrs("reward", "vf_pred", "vf_next", "terminated", "truncated", "advantage", "value_target")),
    "phx_gae_masked": dict(T=4, N=8, gamma=0.5, lambda_=0.25,
                           **ptrs("reward", "vf_pred", "vf_next", "terminated", "truncated", "acted", "reward_valid", "advantage",
                                  "value_target", "reward_sum")),
    "phx_vtrace": dict(T=4, N=8, gamma=0.5, lambda_=0.25, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0,
                       **ptrs("reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp", "terminated", "truncated", "vs", "pg_advantage")),
    "phx_traj_next": dict(T=4, D=3, N=8, **ptrs("truncated", "terminated", "acted", "new_obs_valid", "obs", "new_obs", "next_row",
                                                 "next_terminated", "next_truncated", "next_obs")),
    "phx_traj_compact": dict(T=4, n_planes=2, N=8, capacity=16, **ptrs("keep", "start", "out_row", "out_col"),
                             **{"plane[0].src": A(20), "plane[0].dst": A(21), "plane[0].elem_bytes": 4,
                                "plane[1].src": A(22), "plane[1].dst": A(23), "plane[1].elem_bytes": 1}),
    "phx_nstep": dict(T=4, D=3, N=8, n=3, gamma=0.5,
                      **ptrs("reward", "truncated", "terminated", "acted", "next_row", "next_obs", "succ_row", "nstep_reward", "nstep_discount",
                             "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row", "nstep_next_obs")),
    "phx_episode_stats": dict(T=4, G=2, N=8, K=2, **ptrs("reward", "truncated", "terminated", "acted", "reward_valid", "carry_return",
                                                        "carry_len", "episode_return", "episode_len", "col_stats", "summary")),
    "phx_train_batch": dict(BATCH, **ptrs("keep", "col_class", "start", "records", "out_row", "out_col", "moments", "workspace")),
    "phx_seq_batch": dict(BATCH, max_seq_len=4, **ptrs("keep", "col_class", "seq_start", "records", "out_row", "out_col", "moments", "workspace",
                                                       "terminated", "truncated", "seq_lens", "seq_row", "seq_col")),
    "phx_replay_add": dict(capacity=16, src_capacity=8, count=4, row_words=8, count_ptr=0, src=A(1), ring=A(2), state=A(3)),
    "phx_replay_sample": dict(capacity=16, n=4, row_words=8, seed=1, draw=2, **ptrs("slot_in", "ring", "state", "out", "out_slot")),
    "phx_prio_add": dict(capacity=16, src_capacity=8, count=4, count_ptr=0, ring_state=A(1), tree=A(2), state=A(3)),
    "phx_prio_update": dict(capacity=16, n=4, **ptrs("slot_in", "priority", "ring_state", "tree", "state")),
    "phx_prio_sample": dict(capacity=16, n=4, seed=1, draw=2, **ptrs("ring_state", "tree", "out_slot", "out_priority")),
    "phx_filter_update": dict(T=4, D=3, N=8, n_classes=2, **ptrs("obs", "keep", "col_class", "state", "workspace")),
    "phx_filter_apply": dict(T=4, D=3, N=8, n_classes=2, clip=5.0, **ptrs("obs", "keep", "col_class", "state", "out")),
}


def off(fn, name, by):
    """the good io's pointer `name`, `by` bytes further"""
    return {name: GOOD[fn][name] + by}


def required(fn, names, text):
    return [({n: 0}, text) for n in names]


def aligned(fn, names, by, text):
    return [(off(fn, n, by), text) for n in names]


def unit_interval(text):
    """gamma and lambda, out of range and NaN; `text` takes the two printed values"""
    return [({"gamma": 1.5}, text % ("1.5", "0.25")), ({"gamma": -0.5}, text % ("-0.5", "0.25")), ({"gamma": NAN}, text % ("nan", "0.25")),
            ({"lambda_": 1.5}, text % ("0.5", "1.5")), ({"lambda_": -0.5}, text % ("0.5", "-0.5")), ({"lambda_": NAN}, text % ("0.5", "nan"))]


def rows_cols(grid=True):
    return [({"T": 0}, "T = 0 and N = 8 must be >= 1"), ({"N": 0}, "T = 4 and N = 0 must be >= 1"), ({"T": -1, "N": -1}, "T = -1 and N = -1 must be >= 1")] + \
        ([({"N": GRID64}, "N = 137438953409 is beyond one launch's grid")] if grid else [])


GAE_INTERVAL = "gamma = %s and lambda = %s must lie in [0, 1]"
ROW_WORDS = [({"row_words": 0}, "row_words = 0 must be a multiple of 4 in [4, 256]"), ({"row_words": 260}, "row_words = 260 must be a multiple of 4 in [4, 256]"),
             ({"row_words": 6}, "row_words = 6 must be a multiple of 4 in [4, 256]")]
ELEM_BYTES = "plane 0: elem_bytes = %d must be 1 or 4 * w with 1 <= w <= 64"


def batch_cases():
    """the cases phx_train_batch and phx_seq_batch share: `head` up to S, `planes` from the plane loop to the moments"""
    head = [({"T": 0}, "T = 0 and N = 8 must be >= 1"), ({"N": 0}, "T = 4 and N = 0 must be >= 1"),
            ({"T": 2 ** 31}, "T = 2147483648 must be <= 2^31 - 1"),
            ({"N": 2 ** 60 + 1}, "T * N = 4 * 1152921504606846977 must be <= 2^62"),
            ({"T": 1, "N": GRID64}, "N = 137438953409 is beyond one launch's grid"),
            ({"S": 0}, "S = 0 must be >= 1 and divide N = 8"), ({"S": 3}, "S = 3 must be >= 1 and divide N = 8")]
    planes = [({"plane[0].src": 0}, "plane 0 needs src"), ({"plane[1].src": 0}, "plane 1 needs src"),
              ({"plane[0].elem_bytes": 2}, ELEM_BYTES % 2), ({"plane[0].elem_bytes": 260}, ELEM_BYTES % 260), ({"plane[0].elem_bytes": 6}, ELEM_BYTES % 6),
              ({"plane[0].src": A(20) + 2}, "plane 0: src must be 4-byte aligned"),
              ({"plane[0].word_off": -1}, "plane 0: words [-1, 0) lie outside the record of 8"),
              ({"plane[0].word_off": 8}, "plane 0: words [8, 9) lie outside the record of 8"),
              ({"plane[0].elem_bytes": 36}, "plane 0: words [0, 9) lie outside the record of 8"),
              ({"plane[1].word_off": 0}, "plane 1 overlaps another plane at word 0"),
              ({"plane[0].elem_bytes": 8}, "plane 1 overlaps another plane at word 1"),
              ({"std_plane": -2}, "std_plane = -2 must be -1 or a plane index below 2"), ({"std_plane": 2}, "std_plane = 2 must be -1 or a plane index below 2"),
              ({"std_plane": 1}, "std_plane = 1 must name a plane with elem_bytes 4"),
              ({"moments": 0}, "std_plane needs moments and workspace"), ({"workspace": 0}, "std_plane needs moments and workspace")]
    return head, planes


BATCH_HEAD, BATCH_PLANES_CASES = batch_cases()
N_PLANES = [({"n_planes": -1}, "n_planes = -1 must lie in [0, 32]"), ({"n_planes": 33}, "n_planes = 33 must lie in [0, 32]")]
BATCH_FLAGS = [({"shuffle": 2}, "shuffle = 2 must be 0 or 1"), ({"shuffle": -1}, "shuffle = -1 must be 0 or 1"),
               ({"reserved[0]": 1}, "reserved must be 0"), ({"reserved[1]": 1}, "reserved must be 0")]
COUNT = [({"count": -1}, "count = -1 must lie in [0, src_capacity = 8]"), ({"count": 9}, "count = 9 must lie in [0, src_capacity = 8]")]
PRIO_CAPACITY = [({"capacity": 0}, "capacity = 0 must lie in [1, 2^30]"), ({"capacity": 2 ** 30 + 1}, "capacity = 1073741825 must lie in [1, 2^30]")]
PRIO_N = [({"n": 0}, "n = 0 must be >= 1"), ({"n": GRID256}, "n = 549755813633 is beyond one launch's grid")]
RESERVED2 = [({"reserved[0]": 1}, "reserved must be 0"), ({"reserved[1]": 1}, "reserved must be 0")]
RESERVED3 = [({"reserved0": 1}, "reserved must be 0")] + RESERVED2


def filter_cases(fn):
    return rows_cols(grid=False) + [
        ({"D": 0}, "D = 0 must lie in [1, 16]"), ({"D": 17}, "D = 17 must lie in [1, 16]"),
        ({"n_classes": 0}, "n_classes = 0 must lie in [1, 16]"), ({"n_classes": 17}, "n_classes = 17 must lie in [1, 16]"),
        ({"obs": 0}, "obs and state are required"), ({"state": 0}, "obs and state are required"),
        (off(fn, "obs", 4), "obs and state must be 16-byte aligned"), (off(fn, "state", 8), "obs and state must be 16-byte aligned"),
        (off(fn, "col_class", 2), "col_class must be 4-byte aligned")]


# per entry point: (patch of the good io, the refusal's text after "<entry point>: "), in the order of the entry point's checks
CASES = {
    "phx_gae": [({"reserved0": 1}, "reserved0 must be 0")] + rows_cols() + unit_interval(GAE_INTERVAL)
    + required("phx_gae", ("reward", "truncated", "advantage"), "reward, truncated and advantage are required")
    + aligned("phx_gae", ("reward", "vf_pred", "vf_next"), 2, "reward, vf_pred and vf_next must be 4-byte aligned")
    + aligned("phx_gae", ("advantage", "value_target"), 4, "advantage and value_target must be 16-byte aligned"),

    "phx_gae_masked": [({"reserved0": 1}, "reserved0 must be 0")] + rows_cols() + unit_interval(GAE_INTERVAL)
    + required("phx_gae_masked", ("reward", "truncated", "advantage"), "reward, truncated and advantage are required")
    + aligned("phx_gae_masked", ("reward", "vf_pred", "vf_next"), 2, "reward, vf_pred and vf_next must be 4-byte aligned")
    + aligned("phx_gae_masked", ("advantage", "value_target", "reward_sum"), 8, "advantage, value_target and reward_sum must be 16-byte aligned"),

    "phx_vtrace": [({"reserved0": 1}, "reserved0 and reserved1 must be 0"), ({"reserved1": 1.0}, "reserved0 and reserved1 must be 0"),
                   ({"reserved1": NAN}, "reserved0 and reserved1 must be 0")] + rows_cols() + unit_interval(GAE_INTERVAL)
    + [({"rho_bar": 0.0}, "rho_bar = 0, c_bar = 1 and pg_rho_bar = 1 must be finite and > 0"),
       ({"rho_bar": NAN}, "rho_bar = nan, c_bar = 1 and pg_rho_bar = 1 must be finite and > 0"),
       ({"c_bar": -1.0}, "rho_bar = 1, c_bar = -1 and pg_rho_bar = 1 must be finite and > 0"),
       ({"c_bar": INF}, "rho_bar = 1, c_bar = inf and pg_rho_bar = 1 must be finite and > 0"),
       ({"pg_rho_bar": 0.0}, "rho_bar = 1, c_bar = 1 and pg_rho_bar = 0 must be finite and > 0"),
       ({"pg_rho_bar": NAN}, "rho_bar = 1, c_bar = 1 and pg_rho_bar = nan must be finite and > 0")]
    + required("phx_vtrace", ("reward", "vf_pred", "behaviour_logp", "target_logp", "truncated", "vs"),
               "reward, vf_pred, behaviour_logp, target_logp, truncated and vs are required")
    + aligned("phx_vtrace", ("reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp"), 2,
              "reward, vf_pred, vf_next, behaviour_logp and target_logp must be 4-byte aligned")
    + aligned("phx_vtrace", ("vs", "pg_advantage"), 4, "vs and pg_advantage must be 16-byte aligned"),

    "phx_traj_next": rows_cols()
    + required("phx_traj_next", ("truncated", "next_row", "next_terminated", "next_truncated"),
               "truncated, next_row, next_terminated and next_truncated are required")
    + required("phx_traj_next", ("obs", "new_obs"), "next_obs needs both obs and new_obs")
    + [({"D": 0}, "D = 0 must lie in [1, 64] when next_obs is given"), ({"D": 65}, "D = 65 must lie in [1, 64] when next_obs is given"),
       ({"N": GRID64 - 1, "D": 64}, "N = 137438953408 with D = 64 is beyond one launch's grid")]
    + aligned("phx_traj_next", ("obs", "new_obs"), 2, "obs and new_obs must be 4-byte aligned")
    + aligned("phx_traj_next", ("next_row", "next_terminated", "next_truncated", "next_obs"), 4,
              "next_row, next_terminated, next_truncated and next_obs must be 16-byte aligned")
    + [({"next_obs": 0, "next_terminated": A(7) + 1}, "next_row, next_terminated, next_truncated and next_obs must be 16-byte aligned")],

    "phx_traj_compact": rows_cols()
    + [({"n_planes": -1}, "n_planes = -1 must lie in [0, 16]"), ({"n_planes": 17}, "n_planes = 17 must lie in [0, 16]"),
       ({"capacity": -1}, "capacity = -1 must be >= 0"),
       ({"keep": 0}, "keep and start are required"), ({"start": 0}, "keep and start are required"),
       ({"N": 2 ** 31}, "out_col needs N = 2147483648 <= 2^31 - 1"),
       ({"plane[0].src": 0}, "plane 0 needs src and dst"), ({"plane[1].dst": 0}, "plane 1 needs src and dst"),
       ({"plane[0].elem_bytes": 2}, ELEM_BYTES % 2), ({"plane[0].elem_bytes": 260}, ELEM_BYTES % 260), ({"plane[0].elem_bytes": 6}, ELEM_BYTES % 6),
       ({"plane[0].elem_bytes": 0}, ELEM_BYTES % 0),
       ({"plane[1].reserved": 1}, "plane 1: reserved must be 0"),
       ({"plane[0].src": A(20) + 2}, "plane 0: src must be 4-byte aligned")]
    + aligned("phx_traj_compact", ("start", "out_row", "out_col"), 8, "start, out_row, out_col and every dst must be 16-byte aligned")
    + [({"plane[0].dst": A(21) + 4}, "start, out_row, out_col and every dst must be 16-byte aligned"),
       ({"plane[1].dst": A(23) + 1}, "start, out_row, out_col and every dst must be 16-byte aligned")],

    "phx_nstep": rows_cols()
    + [({"n": 0}, "n = 0 must lie in [1, 64]"), ({"n": 65}, "n = 65 must lie in [1, 64]"),
       ({"gamma": 1.5}, "gamma = 1.5 must lie in [0, 1]"), ({"gamma": -0.5}, "gamma = -0.5 must lie in [0, 1]"),
       ({"gamma": NAN}, "gamma = nan must lie in [0, 1]")]
    + required("phx_nstep", ("reward", "truncated"), "reward and truncated are required")
    + required("phx_nstep", ("nstep_reward", "nstep_discount", "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row"),
               "nstep_reward, nstep_discount, nstep_last, nstep_terminated, nstep_truncated and nstep_next_row are required")
    + [({"succ_row": 0}, "acted needs succ_row"), ({"next_obs": 0}, "nstep_next_obs needs next_obs"),
       ({"D": 0}, "D = 0 must lie in [1, 64] when nstep_next_obs is given"), ({"D": 65}, "D = 65 must lie in [1, 64] when nstep_next_obs is given"),
       ({"N": GRID64 - 1, "D": 64}, "N = 137438953408 with D = 64 is beyond one launch's grid")]
    + aligned("phx_nstep", ("reward", "next_row", "next_obs"), 2, "reward, next_row and next_obs must be 4-byte aligned")
    + aligned("phx_nstep", ("succ_row", "nstep_reward", "nstep_discount", "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row",
                            "nstep_next_obs"), 8, "succ_row and the nstep_ outputs must be 16-byte aligned"),

    "phx_episode_stats": [({"reserved0": 1}, "reserved0 must be 0")] + rows_cols(grid=False)
    + [({"G": 0}, "G = 0 must lie in [1, 256]"), ({"G": 257}, "G = 257 must lie in [1, 256]"),
       ({"N": 9}, "N = 9 must be a multiple of G = 2"),
       ({"K": 0}, "K = 0 must be >= 1 and divide the 4 output columns"), ({"K": 3}, "K = 3 must be >= 1 and divide the 4 output columns"),
       ({"G": 1, "K": 1, "N": GRID64}, "137438953409 output columns are beyond one launch's grid")]
    + required("phx_episode_stats", ("reward", "truncated", "col_stats"), "reward, truncated and col_stats are required")
    + required("phx_episode_stats", ("carry_return", "carry_len"), "carry_return and carry_len come together")
    + aligned("phx_episode_stats", ("reward", "carry_return", "carry_len"), 2, "reward, carry_return and carry_len must be 4-byte aligned")
    + aligned("phx_episode_stats", ("episode_return", "episode_len", "col_stats", "summary"), 8,
              "episode_return, episode_len, col_stats and summary must be 16-byte aligned"),

    "phx_train_batch": BATCH_HEAD + N_PLANES + ROW_WORDS + [({"capacity": -1}, "capacity = -1 must be >= 0")] + BATCH_FLAGS
    + [({"start": 0}, "start is required"), ({"records": 0}, "records is required with n_planes > 0"),
       ({"N": 2 ** 31}, "out_col needs N = 2147483648 <= 2^31 - 1")] + BATCH_PLANES_CASES
    + aligned("phx_train_batch", ("start", "records", "out_row", "out_col", "moments", "workspace"), 8,
              "start, records, out_row, out_col, moments and workspace must be 16-byte aligned"),

    "phx_seq_batch": BATCH_HEAD
    + [({"max_seq_len": 0}, "max_seq_len = 0 must lie in [1, 65536]"), ({"max_seq_len": 65537}, "max_seq_len = 65537 must lie in [1, 65536]")]
    + N_PLANES + ROW_WORDS
    + [({"capacity": -1}, "capacity = -1 must be >= 0"),
       ({"capacity": 2 ** 60 + 1}, "capacity * max_seq_len = 1152921504606846977 * 4 must be <= 2^62")] + BATCH_FLAGS
    + [({"seq_start": 0}, "seq_start is required"), ({"records": 0}, "records is required with n_planes > 0"),
       ({"N": 2 ** 31, "seq_col": 0}, "out_col and seq_col need N = 2147483648 <= 2^31 - 1"),
       ({"N": 2 ** 31, "out_col": 0}, "out_col and seq_col need N = 2147483648 <= 2^31 - 1")] + BATCH_PLANES_CASES
    + aligned("phx_seq_batch", ("seq_start", "records", "out_row", "out_col", "moments", "workspace", "seq_lens", "seq_row", "seq_col"), 8,
              "seq_start, records, out_row, out_col, seq_lens, seq_row, seq_col, moments and workspace must be 16-byte aligned"),

    "phx_replay_add": [({"capacity": 0}, "capacity = 0 must be >= 1"), ({"src_capacity": -1}, "src_capacity = -1 must be >= 0")] + ROW_WORDS + RESERVED3 + COUNT
    + required("phx_replay_add", ("ring", "state"), "ring and state are required")
    + [({"src": 0}, "src is required with src_capacity > 0")]
    + aligned("phx_replay_add", ("src", "ring", "state"), 8, "src, ring and state must be 16-byte aligned")
    + [({"count_ptr": A(0) + 4}, "count_ptr must be 8-byte aligned"),
       ({"src_capacity": 512 * 0x7fffffff + 1}, "src_capacity = 1099511627265 is beyond one launch's grid")],

    "phx_replay_sample": [({"capacity": 0}, "capacity = 0 must be >= 1"), ({"n": 0}, "n = 0 must be >= 1")] + ROW_WORDS + RESERVED3
    + required("phx_replay_sample", ("ring", "state", "out"), "ring, state and out are required")
    + aligned("phx_replay_sample", ("ring", "state", "out", "out_slot"), 8, "ring, state, out and out_slot must be 16-byte aligned")
    + [(off("phx_replay_sample", "slot_in", 4), "slot_in must be 8-byte aligned"),
       ({"n": 512 * 0x7fffffff + 1}, "n = 1099511627265 is beyond one launch's grid")],

    "phx_prio_add": PRIO_CAPACITY + [({"src_capacity": -1}, "src_capacity = -1 must be >= 0")] + RESERVED2 + COUNT
    + required("phx_prio_add", ("ring_state", "tree", "state"), "ring_state, tree and state are required")
    + aligned("phx_prio_add", ("tree", "state"), 8, "tree and state must be 16-byte aligned")
    + [({"count_ptr": A(0) + 4}, "count_ptr and ring_state must be 8-byte aligned"),
       (off("phx_prio_add", "ring_state", 4), "count_ptr and ring_state must be 8-byte aligned")],

    "phx_prio_update": PRIO_CAPACITY + PRIO_N + RESERVED2
    + required("phx_prio_update", ("slot_in", "priority", "ring_state", "tree", "state"), "slot_in, priority, ring_state, tree and state are required")
    + aligned("phx_prio_update", ("tree", "state"), 8, "tree and state must be 16-byte aligned")
    + aligned("phx_prio_update", ("slot_in", "ring_state"), 4, "slot_in and ring_state must be 8-byte aligned")
    + [(off("phx_prio_update", "priority", 2), "priority must be 4-byte aligned")],

    "phx_prio_sample": PRIO_CAPACITY + PRIO_N + RESERVED2
    + required("phx_prio_sample", ("ring_state", "tree", "out_slot", "out_priority"), "ring_state, tree, out_slot and out_priority are required")
    + aligned("phx_prio_sample", ("tree", "out_slot", "out_priority"), 8, "tree, out_slot and out_priority must be 16-byte aligned")
    + [(off("phx_prio_sample", "ring_state", 4), "ring_state must be 8-byte aligned")],

    "phx_filter_update": [({"reserved0": 1}, "the reserved fields must be 0"), ({"reserved[0]": 1}, "the reserved fields must be 0"),
                          ({"reserved[1]": 1}, "the reserved fields must be 0")] + filter_cases("phx_filter_update")
    + [({"workspace": 0}, "workspace is required and must be 16-byte aligned"),
       (off("phx_filter_update", "workspace", 8), "workspace is required and must be 16-byte aligned"),
       ({"N": GRID64}, "137438953409 columns are beyond one launch's grid")],

    "phx_filter_apply": [({"reserved[0]": 1}, "the reserved fields must be 0"), ({"reserved[1]": 1}, "the reserved fields must be 0")]
    + filter_cases("phx_filter_apply")
    + [({"out": 0}, "out is required and must be 16-byte aligned"), (off("phx_filter_apply", "out", 8), "out is required and must be 16-byte aligned"),
       ({"clip": -1.0}, "clip = -1 must be >= 0 (0: none)"), ({"clip": NAN}, "clip = nan must be >= 0 (0: none)"),
       ({"N": 2 ** 31}, "T = 4 rows of N = 2147483648 columns are beyond one launch's grid"),
       ({"T": 8192, "N": 2 ** 26, "D": 16}, "T = 8192 rows of N = 67108864 columns are beyond one launch's grid"),
       ({"out": A(0) + 16}, "out overlaps obs in part (out == obs, exactly in place, is allowed)"),
       ({"out": A(0) - 16}, "out overlaps obs in part (out == obs, exactly in place, is allowed)")],
}

# two rules broken at once, adjacent in the entry point's check order: the earlier one's text
_BATCH_PAIRS_TAIL = [
    ({"n_planes": -1, "row_words": 0}, "n_planes = -1 must lie in [0, 32]"),
    ({"row_words": 0, "capacity": -1}, "row_words = 0 must be a multiple of 4 in [4, 256]"),
    ({"capacity": -1, "shuffle": 2}, "capacity = -1 must be >= 0"),
    ({"shuffle": 2, "reserved[0]": 1}, "shuffle = 2 must be 0 or 1")]
_PLANE_PAIRS = [
    ({"plane[0].src": 0, "plane[0].elem_bytes": 2}, "plane 0 needs src"),
    ({"plane[0].elem_bytes": 6, "plane[0].src": A(20) + 2}, ELEM_BYTES % 6),
    ({"plane[0].src": A(20) + 2, "plane[0].word_off": -1}, "plane 0: src must be 4-byte aligned"),
    ({"plane[0].word_off": 8, "plane[1].word_off": 8}, "plane 0: words [8, 9) lie outside the record of 8"),
    ({"plane[1].word_off": 0, "std_plane": -2}, "plane 1 overlaps another plane at word 0"),
    ({"std_plane": 2, "moments": 0}, "std_plane = 2 must be -1 or a plane index below 2"),
    ({"std_plane": 1, "moments": 0}, "std_plane = 1 must name a plane with elem_bytes 4")]
PAIRS = {
    "phx_train_batch": [
        ({"N": 0, "T": 2 ** 31}, "T = 2147483648 and N = 0 must be >= 1"),
        ({"T": 2 ** 31, "N": 2 ** 60}, "T = 2147483648 must be <= 2^31 - 1"),
        ({"N": 2 ** 61}, "T * N = 4 * 2305843009213693952 must be <= 2^62"),
        ({"T": 1, "N": GRID64, "S": 0}, "N = 137438953409 is beyond one launch's grid"),
        ({"S": 0, "n_planes": -1}, "S = 0 must be >= 1 and divide N = 8")] + _BATCH_PAIRS_TAIL
    + [({"reserved[0]": 1, "start": 0}, "reserved must be 0"),
       ({"start": 0, "records": 0}, "start is required"),
       ({"records": 0, "N": 2 ** 31}, "records is required with n_planes > 0"),
       ({"N": 2 ** 31, "plane[0].src": 0}, "out_col needs N = 2147483648 <= 2^31 - 1")] + _PLANE_PAIRS
    + [({"moments": 0, "start": A(2) + 8}, "std_plane needs moments and workspace")],

    "phx_seq_batch": [
        ({"N": 0, "T": 2 ** 31}, "T = 2147483648 and N = 0 must be >= 1"),
        ({"T": 2 ** 31, "N": 2 ** 60}, "T = 2147483648 must be <= 2^31 - 1"),
        ({"N": 2 ** 61}, "T * N = 4 * 2305843009213693952 must be <= 2^62"),
        ({"T": 1, "N": GRID64, "S": 0}, "N = 137438953409 is beyond one launch's grid"),
        ({"S": 0, "max_seq_len": 0}, "S = 0 must be >= 1 and divide N = 8"),
        ({"max_seq_len": 0, "n_planes": -1}, "max_seq_len = 0 must lie in [1, 65536]")] + _BATCH_PAIRS_TAIL[:3]
    + [({"capacity": 2 ** 60 + 1, "shuffle": 2}, "capacity * max_seq_len = 1152921504606846977 * 4 must be <= 2^62"), _BATCH_PAIRS_TAIL[3],
       ({"reserved[0]": 1, "seq_start": 0}, "reserved must be 0"),
       ({"seq_start": 0, "records": 0}, "seq_start is required"),
       ({"records": 0, "N": 2 ** 31}, "records is required with n_planes > 0"),
       ({"N": 2 ** 31, "plane[0].src": 0}, "out_col and seq_col need N = 2147483648 <= 2^31 - 1")] + _PLANE_PAIRS
    + [({"moments": 0, "seq_start": A(2) + 8}, "std_plane needs moments and workspace")],

    "phx_replay_add": [
        ({"capacity": 0, "src_capacity": -1}, "capacity = 0 must be >= 1"),
        ({"src_capacity": -1, "row_words": 0}, "src_capacity = -1 must be >= 0"),
        ({"row_words": 0, "reserved0": 1}, "row_words = 0 must be a multiple of 4 in [4, 256]"),
        ({"reserved0": 1, "count": -1}, "reserved must be 0"),
        ({"count": -1, "ring": 0}, "count = -1 must lie in [0, src_capacity = 8]"),
        ({"ring": 0, "src": 0}, "ring and state are required"),
        ({"src": 0, "state": A(3) + 8}, "src is required with src_capacity > 0"),
        ({"state": A(3) + 8, "count_ptr": A(0) + 4}, "src, ring and state must be 16-byte aligned"),
        ({"count_ptr": A(0) + 4, "src_capacity": 512 * 0x7fffffff + 1}, "count_ptr must be 8-byte aligned")],

    "phx_prio_add": [
        ({"capacity": 0, "src_capacity": -1}, "capacity = 0 must lie in [1, 2^30]"),
        ({"src_capacity": -1, "reserved[0]": 1}, "src_capacity = -1 must be >= 0"),
        ({"reserved[0]": 1, "count": -1}, "reserved must be 0"),
        ({"count": -1, "tree": 0}, "count = -1 must lie in [0, src_capacity = 8]"),
        ({"tree": 0, "state": A(3) + 8}, "ring_state, tree and state are required"),
        ({"state": A(3) + 8, "ring_state": A(1) + 4}, "tree and state must be 16-byte aligned")],
}

ALL = [(fn, patch, text) for table in (CASES, PAIRS) for fn, cases in table.items() for patch, text in cases]


def make(fn, patch):
    io = OPS[fn]()
    for key, value in {**GOOD[fn], **patch}.items():
        m = re.fullmatch(r"(\w+)\[(\d+)\](?:\.(\w+))?", key)
        if not m:
            setattr(io, key, value)
        elif m.group(3):
            setattr(getattr(io, m.group(1))[int(m.group(2))], m.group(3), value)
        else:
            getattr(io, m.group(1))[int(m.group(2))] = value
    return io


def refuse(lib, fn, patch):
    rc = getattr(lib, fn)(C.byref(make(fn, patch)), None)
    return rc, lib.phx_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


@pytest.mark.parametrize("fn,patch,text", ALL, ids=[f"{fn}-{i}" for i, (fn, _, _) in enumerate(ALL)])
def test_the_refusal_verbatim(lib, fn, patch, text):
    rc, said = refuse(lib, fn, patch)
    assert rc == PHX_EINVAL, (rc, said)
    assert said == f"{fn}: {text}"


@pytest.mark.parametrize("fn", sorted(OPS))
def test_a_null_io(lib, fn):
    rc = getattr(lib, fn)(None, None)
    assert rc == PHX_EINVAL
    assert lib.phx_last_error().decode() == f"{fn}: null io"


def test_every_entry_point_has_its_cases():
    assert set(CASES) == set(GOOD) == set(OPS) and len(OPS) == 16
    assert all(len(c) >= 10 for c in CASES.values())


def test_refusals_leave_phx_last_kernel_as_it_was(lib):
    before = lib.phx_last_kernel()
    for fn, patch, _ in ALL:
        assert refuse(lib, fn, patch)[0] == PHX_EINVAL, (fn, patch)
    for fn in OPS:
        assert getattr(lib, fn)(None, None) == PHX_EINVAL
    assert lib.phx_last_kernel() == before
