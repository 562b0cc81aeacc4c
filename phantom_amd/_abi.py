"""ctypes mirror of include/phantom_amd.h and the loader of libphantom_amd.so.

The product path has no CPU fallback: if the HIP library is missing, ``load_library`` raises.
"""
import ctypes as C
import os

ABI_VERSION = 10
NPI, NPF = 4, 8

# phx_kind
KIND_FACTORY, KIND_SHOP, KIND_CUSTOMER, KIND_SELLER, KIND_BUYER = 1, 2, 3, 4, 5
KIND_HALVER, KIND_CASHBOX, KIND_REQRESP, KIND_FORWARDER = 6, 7, 8, 9
KIND_MOCK_STRAT, KIND_MOCK_AGENT = 10, 11
KIND_PUBLISHER, KIND_ADVERTISER, KIND_ADEXCHANGE = 12, 13, 14
KIND_NAMES = {1: "factory", 2: "shop", 3: "customer", 4: "seller", 5: "buyer", 6: "halver",
              7: "cashbox", 8: "reqresp", 9: "forwarder", 10: "mock", 11: "mock_agent",
              12: "pub", 13: "adv", 14: "adx"}
STRATEGIC_KINDS = (KIND_SHOP, KIND_SELLER, KIND_BUYER, KIND_MOCK_STRAT, KIND_ADVERTISER)
OBS_DIM = {KIND_SHOP: 3, KIND_SELLER: 2, KIND_BUYER: 2, KIND_MOCK_STRAT: 1, KIND_ADVERTISER: 3}

# phx_msg_type
(MSG_STOCK_REQUEST, MSG_STOCK_RESPONSE, MSG_ORDER_REQUEST, MSG_ORDER_RESPONSE, MSG_PRICE,
 MSG_ORDER, MSG_HALVE, MSG_CASH, MSG_REQUEST, MSG_RESPONSE, MSG_PING) = range(1, 12)
(MSG_IMPRESSION_REQ, MSG_BID, MSG_AUCTION_RESULT, MSG_ADS, MSG_IMPRESSION_RES) = range(12, 17)
FLOAT_PAYLOAD_TYPES = (MSG_PRICE, MSG_CASH, MSG_REQUEST, MSG_RESPONSE, MSG_BID, MSG_AUCTION_RESULT)
TAG_PYF, TAG_F32, TAG_F64 = 0, 1, 2      # PHX_TAG_*: numpy scalar kind of an ads-market float

ENV_PLAIN, ENV_FSM, ENV_STACKELBERG = 0, 1, 2
# phx_spec.variant_* (ABI 6)
VR_AUTO, VR_TIME_PARALLEL, VR_LEAN, VR_GENERAL, VR_LAUNCH_LOOP, VR_STORE_WAVES = 0, 1, 2, 3, 4, 5
VR_POLICY_MFMA = 6
VB_WHOLE_ENVS = -1
VS_AUTO, VS_FUSED, VS_GENERIC, VS_WIDE, VS_GENERIC_DYNAMIC = 0, 1, 2, 3, 4
SAMPLER_HOST, SAMPLER_UNIFORM = 0, 1
TYPE_NONE, TYPE_CONST = -2, -1
F_IGNORE_CONN_ERRORS, F_NO_PAYLOAD_CHECKS, F_FORCE_GENERIC, F_SHUFFLE_BATCHES, F_MT19937 = 1, 2, 4, 8, 16

(ERR_NONE, ERR_NETWORK, ERR_PAYLOAD, ERR_UNKNOWN_MSG, ERR_ROUND_LIMIT, ERR_QUEUE_FULL,
 ERR_CONTEXT, ERR_FSM_TRANSITION, ERR_HINT) = range(9)
MAX_ROUNDS = 4096            # PHX_MAX_ROUNDS: cap on BatchResolver(round_limit=None) rounds

_u8p, _i32p, _f32p, _f64p = (C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                             C.POINTER(C.c_double))


class PhxSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_agents", C.c_int32), ("batch", C.c_int32),
        ("num_steps", C.c_int32), ("round_limit", C.c_int32), ("env_type", C.c_int32),
        ("flags", C.c_uint32), ("queue_cap", C.c_int32), ("trace_cap", C.c_int32),
        ("kind", C.c_void_p), ("param_i", C.c_void_p), ("param_f", C.c_void_p),
        ("row_ptr", C.c_void_p), ("col", C.c_void_p),
        ("n_stages", C.c_int32), ("initial_stage", C.c_int32),
        ("stage_act_ptr", C.c_void_p), ("stage_act_idx", C.c_void_p),
        ("stage_rewarded", C.c_void_p), ("stage_rewarded_all", C.c_void_p),
        ("stage_next", C.c_void_p),
        ("n_leaders", C.c_int32), ("n_followers", C.c_int32),
        ("leaders", C.c_void_p), ("followers", C.c_void_p),
        ("seed", C.c_uint64), ("env_offset", C.c_int64),
        ("n_samplers", C.c_int32), ("sampler_kind", C.c_void_p), ("sampler_param", C.c_void_p),
        ("type_src", C.c_void_p),
        ("n_conn", C.c_int32), ("conn_rate", C.c_void_p), ("col_conn", C.c_void_p),
        ("stage_allowed", C.c_void_p),
        ("variant_rollout", C.c_int32), ("variant_block", C.c_int32), ("variant_step", C.c_int32),
        ("variant_reserved", C.c_int32),
        ("stage_tab", C.c_void_p),
        ("n_stage_rules", C.c_int32), ("reserved1", C.c_int32), ("stage_rules", C.c_void_p),
    ]


class PhxField(C.Structure):
    _fields_ = [("field_id", C.c_int32), ("dtype", C.c_int32), ("offset", C.c_int64),
                ("dim0", C.c_int32), ("dim1", C.c_int32), ("dim2", C.c_int32),
                ("kind", C.c_int32), ("name", C.c_char * 32)]


class _Payload(C.Union):
    _fields_ = [("i", C.c_int64), ("f", C.c_double)]


class PhxMsgRec(C.Structure):
    _fields_ = [("sender", C.c_uint16), ("receiver", C.c_uint16), ("type", C.c_uint16),
                ("round", C.c_uint16), ("payload", _Payload)]


class PhxStepIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "actions", "action_valid", "exo", "obs", "obs_valid", "reward", "reward_valid",
        "terminated", "truncated", "done_valid", "all_terminated", "all_truncated", "err",
        "msg_log", "msg_count", "shuffle", "next_stage")]


class PhxRolloutIO(C.Structure):
    _fields_ = [("T", C.c_int32), ("hints", C.c_int32)] + [(n, C.c_void_p) for n in (
        "actions", "exo", "obs", "action_out", "reward", "terminated", "truncated", "obs_valid",
        "reward_valid", "last_obs", "err", "msg_log", "msg_count", "reserved_ptr")] + [
        ("n_frag", C.c_int32), ("reserved0", C.c_int32), ("frags", C.c_void_p), ("policy", C.c_void_p)]


class PhxPolicyMLP(C.Structure):
    """phx_policy_mlp (ABI 10): the device-evaluated policy of a rollout"""
    _fields_ = [("n_hidden", C.c_int32), ("width", C.c_int32 * 2), ("activation", C.c_int32),
                ("out_scale", C.c_float), ("out_bias", C.c_float), ("out_lo", C.c_float), ("out_hi", C.c_float),
                ("w", C.c_void_p * 3), ("b", C.c_void_p * 3)]


class PhxPolicyExplore(C.Structure):
    """phx_policy_explore (ABI 10, additive): Gaussian exploration of the rollout's policy, passed in phx_rollout_io.reserved_ptr"""
    _fields_ = [(n, C.c_void_p) for n in ("noise", "w_log_std", "b_log_std", "raw_action", "logp", "dist_inputs")]


ACT_RELU, ACT_HARD_TANH, ACT_TANH = 0, 1, 2
LOG_STD_MIN, LOG_STD_MAX = -20.0, 20.0
POLICY_MAX_WIDTH = 64
POLICY_WIDE_MAX, POLICY_WIDE_STEP = 256, 32


class PhxStageRule(C.Structure):
    """phx_stage_rule (ABI 9): one rule of a device-evaluated state handler"""
    _fields_ = [("stage", C.c_int32), ("agent", C.c_int32), ("cmp", C.c_int32), ("next_stage", C.c_int32),
                ("threshold", C.c_double), ("field", C.c_char * 32)]


CMP = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}


class PhxRolloutFrag(C.Structure):
    """one fragment of a fragment-list rollout (phx_rollout_io.frags, ABI 9)"""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "action_out", "reward", "terminated", "truncated", "obs_valid", "reward_valid")]


class PhxGaeIO(C.Structure):
    """phx_gae_io (include/phantom_amd_gae.h): the planes of one phx_gae call"""
    _fields_ = [("T", C.c_int32), ("reserved0", C.c_int32), ("N", C.c_int64), ("gamma", C.c_float), ("lambda_", C.c_float)] + [
        (n, C.c_void_p) for n in ("reward", "vf_pred", "vf_next", "terminated", "truncated", "advantage", "value_target")]


class PhxGaeMaskedIO(C.Structure):
    """phx_gae_masked_io (include/phantom_amd_gae.h): the planes of one phx_gae_masked call"""
    _fields_ = [("T", C.c_int32), ("reserved0", C.c_int32), ("N", C.c_int64), ("gamma", C.c_float), ("lambda_", C.c_float)] + [
        (n, C.c_void_p) for n in ("reward", "vf_pred", "vf_next", "terminated", "truncated", "acted", "reward_valid", "advantage",
                                  "value_target", "reward_sum")]


class PhxVtraceIO(C.Structure):
    """phx_vtrace_io (include/phantom_amd_vtrace.h): the planes of one phx_vtrace call"""
    _fields_ = [("T", C.c_int32), ("reserved0", C.c_int32), ("N", C.c_int64), ("gamma", C.c_float), ("lambda_", C.c_float),
                ("rho_bar", C.c_float), ("c_bar", C.c_float), ("pg_rho_bar", C.c_float), ("reserved1", C.c_float)] + [
        (n, C.c_void_p) for n in ("reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp", "terminated", "truncated", "vs",
                                  "pg_advantage")]


class PhxTrajNextIO(C.Structure):
    """phx_traj_next_io (include/phantom_amd_traj.h): the planes of one phx_traj_next call"""
    _fields_ = [("T", C.c_int32), ("D", C.c_int32), ("N", C.c_int64)] + [
        (n, C.c_void_p) for n in ("truncated", "terminated", "acted", "new_obs_valid", "obs", "new_obs", "next_row", "next_terminated",
                                  "next_truncated", "next_obs")]


COMPACT_MAX_PLANES = 16


class PhxCompactPlane(C.Structure):
    """phx_compact_plane (include/phantom_amd_compact.h): one plane of a phx_traj_compact call"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("elem_bytes", C.c_int32), ("reserved", C.c_int32)]


class PhxTrajCompactIO(C.Structure):
    """phx_traj_compact_io (include/phantom_amd_compact.h): the planes of one phx_traj_compact call"""
    _fields_ = [("T", C.c_int32), ("n_planes", C.c_int32), ("N", C.c_int64), ("capacity", C.c_int64), ("keep", C.c_void_p),
                ("start", C.c_void_p), ("out_row", C.c_void_p), ("out_col", C.c_void_p), ("plane", PhxCompactPlane * COMPACT_MAX_PLANES)]


class PhxNstepIO(C.Structure):
    """phx_nstep_io (include/phantom_amd_nstep.h): the planes of one phx_nstep call"""
    _fields_ = [("T", C.c_int32), ("D", C.c_int32), ("N", C.c_int64), ("n", C.c_int32), ("gamma", C.c_float)] + [
        (n, C.c_void_p) for n in ("reward", "truncated", "terminated", "acted", "next_row", "next_obs", "succ_row", "nstep_reward",
                                  "nstep_discount", "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row", "nstep_next_obs")]


class PhxEpisodeStats(C.Structure):
    """struct phx_episode_stats (include/phantom_amd_episodes.h): one element of col_stats / summary"""
    _fields_ = [("count", C.c_int64), ("len_sum", C.c_int64), ("ret_sum", C.c_double), ("ret_sumsq", C.c_double),
                ("ret_min", C.c_float), ("ret_max", C.c_float), ("len_min", C.c_int32), ("len_max", C.c_int32)]


class PhxEpisodeIO(C.Structure):
    """phx_episode_io (include/phantom_amd_episodes.h): the planes of one phx_episode_stats call"""
    _fields_ = [("T", C.c_int32), ("G", C.c_int32), ("N", C.c_int64), ("K", C.c_int32), ("reserved0", C.c_int32)] + [
        (n, C.c_void_p) for n in ("reward", "truncated", "terminated", "acted", "reward_valid", "carry_return", "carry_len",
                                  "episode_return", "episode_len", "col_stats", "summary")]


BATCH_MAX_PLANES = 32


class PhxBatchPlane(C.Structure):
    """phx_batch_plane (include/phantom_amd_batch.h): one plane of a phx_train_batch call"""
    _fields_ = [("src", C.c_void_p), ("elem_bytes", C.c_int32), ("word_off", C.c_int32)]


class PhxBatchMoments(C.Structure):
    """phx_batch_moments (include/phantom_amd_batch.h): the moments of the standardized plane"""
    _fields_ = [("count", C.c_int64), ("sum", C.c_double), ("sumsq", C.c_double), ("mean", C.c_float), ("den", C.c_float)]


class PhxTrainBatchIO(C.Structure):
    """phx_train_batch_io (include/phantom_amd_batch.h): the planes and buffers of one phx_train_batch call"""
    _fields_ = [("T", C.c_int64), ("N", C.c_int64), ("capacity", C.c_int64), ("n_planes", C.c_int32), ("row_words", C.c_int32),
                ("S", C.c_int32), ("class_id", C.c_int32), ("std_plane", C.c_int32), ("shuffle", C.c_int32), ("seed", C.c_uint64),
                ("epoch", C.c_uint64)] + [(n, C.c_void_p) for n in ("keep", "col_class", "start", "records", "out_row", "out_col", "moments",
                                                                    "workspace")] + [("reserved", C.c_int64 * 2),
                                                                                     ("plane", PhxBatchPlane * BATCH_MAX_PLANES)]


class PhxSeqBatchIO(C.Structure):
    """phx_seq_batch_io (include/phantom_amd_seq.h): the planes and buffers of one phx_seq_batch call"""
    _fields_ = [("T", C.c_int64), ("N", C.c_int64), ("capacity", C.c_int64), ("n_planes", C.c_int32), ("row_words", C.c_int32),
                ("S", C.c_int32), ("class_id", C.c_int32), ("std_plane", C.c_int32), ("shuffle", C.c_int32), ("seed", C.c_uint64),
                ("epoch", C.c_uint64)] + [(n, C.c_void_p) for n in ("keep", "col_class", "seq_start", "records", "out_row", "out_col", "moments",
                                                                    "workspace")] + [("max_seq_len", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("terminated", "truncated", "seq_lens", "seq_row", "seq_col")] + [("reserved", C.c_int64 * 2),
                                                                                                          ("plane", PhxBatchPlane * BATCH_MAX_PLANES)]


class PhxReplayState(C.Structure):
    """phx_replay_state (include/phantom_amd_replay.h): the 32 device-resident bytes that go with a ring"""
    _fields_ = [("cursor", C.c_int64), ("size", C.c_int64), ("total", C.c_int64), ("refused", C.c_int64)]


class PhxReplayAddIO(C.Structure):
    """phx_replay_add_io (include/phantom_amd_replay.h): the buffers of one phx_replay_add call"""
    _fields_ = [("capacity", C.c_int64), ("src_capacity", C.c_int64), ("count", C.c_int64), ("row_words", C.c_int32), ("reserved0", C.c_int32)] + [
        (n, C.c_void_p) for n in ("count_ptr", "src", "ring", "state")] + [("reserved", C.c_int64 * 2)]


class PhxReplaySampleIO(C.Structure):
    """phx_replay_sample_io (include/phantom_amd_replay.h): the buffers of one phx_replay_sample call"""
    _fields_ = [("capacity", C.c_int64), ("n", C.c_int64), ("row_words", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64),
                ("draw", C.c_uint64)] + [(n, C.c_void_p) for n in ("slot_in", "ring", "state", "out", "out_slot")] + [("reserved", C.c_int64 * 2)]


class PhxPrioState(C.Structure):
    """phx_prio_state (include/phantom_amd_prio.h): the 32 device-resident bytes that go with a priority tree"""
    _fields_ = [("max_priority", C.c_float), ("reserved0", C.c_uint32), ("ignored", C.c_int64), ("refused", C.c_int64), ("reserved1", C.c_int64)]


class PhxPrioAddIO(C.Structure):
    """phx_prio_add_io (include/phantom_amd_prio.h): the buffers of one phx_prio_add call"""
    _fields_ = [("capacity", C.c_int64), ("src_capacity", C.c_int64), ("count", C.c_int64)] + [
        (n, C.c_void_p) for n in ("count_ptr", "ring_state", "tree", "state")] + [("reserved", C.c_int64 * 2)]


class PhxPrioUpdateIO(C.Structure):
    """phx_prio_update_io (include/phantom_amd_prio.h): the buffers of one phx_prio_update call"""
    _fields_ = [("capacity", C.c_int64), ("n", C.c_int64)] + [
        (n, C.c_void_p) for n in ("slot_in", "priority", "ring_state", "tree", "state")] + [("reserved", C.c_int64 * 2)]


class PhxPrioSampleIO(C.Structure):
    """phx_prio_sample_io (include/phantom_amd_prio.h): the buffers of one phx_prio_sample call"""
    _fields_ = [("capacity", C.c_int64), ("n", C.c_int64), ("seed", C.c_uint64), ("draw", C.c_uint64)] + [
        (n, C.c_void_p) for n in ("ring_state", "tree", "out_slot", "out_priority")] + [("reserved", C.c_int64 * 2)]


class PhxFilterState(C.Structure):
    """phx_filter_state (include/phantom_amd_filter.h): the 272 device-resident bytes of one class of an observation filter"""
    _fields_ = [("count", C.c_int64), ("updates", C.c_int64), ("mean", C.c_double * 16), ("m2", C.c_double * 16)]


class PhxFilterUpdateIO(C.Structure):
    """phx_filter_update_io (include/phantom_amd_filter.h): the buffers of one phx_filter_update call"""
    _fields_ = [("T", C.c_int32), ("D", C.c_int32), ("N", C.c_int64), ("n_classes", C.c_int32), ("reserved0", C.c_int32)] + [
        (n, C.c_void_p) for n in ("obs", "keep", "col_class", "state", "workspace")] + [("reserved", C.c_int64 * 2)]


class PhxFilterApplyIO(C.Structure):
    """phx_filter_apply_io (include/phantom_amd_filter.h): the buffers of one phx_filter_apply call"""
    _fields_ = [("T", C.c_int32), ("D", C.c_int32), ("N", C.c_int64), ("n_classes", C.c_int32), ("clip", C.c_float)] + [
        (n, C.c_void_p) for n in ("obs", "keep", "col_class", "state", "out")] + [("reserved", C.c_int64 * 2)]


SEQ_MAX_LEN = 65536
FILTER_MAX_DIM = 16
FILTER_MAX_CLASSES = 16
# one class's 272 bytes as a numpy record: ndarray.view of a uint8 [n_classes, 272] host copy
FILTER_STATE_DTYPE = [("count", "<i8"), ("updates", "<i8"), ("mean", "<f8", (FILTER_MAX_DIM,)), ("m2", "<f8", (FILTER_MAX_DIM,))]
FILTER_STATE_BYTES = 272


def filter_workspace_bytes(N, D):
    """PHX_FILTER_WORKSPACE_BYTES(N, D) of include/phantom_amd_filter.h: the scratch one phx_filter_update call needs"""
    return 8 * ((int(D) + 1) * int(N) + 528)


# the priority state's 32 bytes as a numpy record: ndarray.view of a uint8 [32] host copy
PRIO_STATE_DTYPE = [("max_priority", "<f4"), ("reserved0", "<u4"), ("ignored", "<i8"), ("refused", "<i8"), ("reserved1", "<i8")]
PRIO_STATE_BYTES = 32
PRIO_FANOUT = 16
PRIO_MAX_CAPACITY = 2 ** 30
PRIO_TOP_NODES = 256                                     # levels of more nodes are served by one launch each, the others by the top kernel


def prio_layout(capacity):
    """``(L, offsets, W, words)`` of the tree over a ring of ``capacity`` slots (include/phantom_amd_prio.h): sum level l starts at
    ``offsets[l]``, min level l >= 1 at ``W + offsets[l] - offsets[1]`` (``offsets[1]`` is w_0; L == 0: there is none), and the
    buffer holds ``words`` f32"""
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= PRIO_MAX_CAPACITY:
        raise ValueError(f"prio_layout: capacity = {capacity!r} must be an int in [1, 2^30]")
    n, offsets = capacity, [0]
    while n != 1:
        w = PRIO_FANOUT * -(-n // PRIO_FANOUT)
        offsets.append(offsets[-1] + w)
        n = w // PRIO_FANOUT
    W = offsets[-1] + PRIO_FANOUT
    return len(offsets) - 1, tuple(offsets), W, 2 * W - PRIO_FANOUT * -(-capacity // PRIO_FANOUT)


def prio_min_root(capacity):
    """the word of the tree buffer that holds pmin, the root of the min tree (L == 0: the one leaf)"""
    L, offsets, W, _ = prio_layout(capacity)
    return W + offsets[L] - offsets[1] if L else 0


# the state's 32 bytes as a numpy record: ndarray.view of an int64 [4] host copy
REPLAY_STATE_DTYPE = [("cursor", "<i8"), ("size", "<i8"), ("total", "<i8"), ("refused", "<i8")]
REPLAY_STATE_BYTES = 32
# the moments' 32 bytes as a numpy record: ndarray.view of a uint8 [32] host copy
BATCH_MOMENTS_DTYPE = [("count", "<i8"), ("sum", "<f8"), ("sumsq", "<f8"), ("mean", "<f4"), ("den", "<f4")]
BATCH_MOMENTS_BYTES = 32

# the same 48 bytes as a numpy record: np.frombuffer / ndarray.view of a uint8 [.., 48] host copy of col_stats / summary
EPISODE_STATS_DTYPE = [("count", "<i8"), ("len_sum", "<i8"), ("ret_sum", "<f8"), ("ret_sumsq", "<f8"), ("ret_min", "<f4"),
                       ("ret_max", "<f4"), ("len_min", "<i4"), ("len_max", "<i4")]
EPISODE_STATS_BYTES = 48
EPISODE_MAX_G = 256

GAE_KERNEL = "phx_gae_kernel"
GAE_MASKED_KERNEL = "phx_gae_masked_kernel"
VTRACE_KERNEL = "phx_vtrace_kernel"
TRAJ_NEXT_KERNEL = "phx_traj_next_kernel"                # (with next_obs: + "+phx_traj_gather_kernel")
TRAJ_GATHER_KERNEL = "phx_traj_gather_kernel"
COMPACT_COUNT_KERNEL = "phx_compact_count_kernel"        # (phx_traj_compact: the three names joined by "+"; the scatter's is missing
COMPACT_SCAN_KERNEL = "phx_compact_scan_kernel"          #  where it has nothing to write)
COMPACT_SCATTER_KERNEL = "phx_compact_scatter_kernel"
COMPACT_KERNELS = "+".join((COMPACT_COUNT_KERNEL, COMPACT_SCAN_KERNEL, COMPACT_SCATTER_KERNEL))
NSTEP_SUCC_KERNEL = "phx_nstep_succ_kernel"              # (phx_nstep: the names of the kernels launched joined by "+"; the scan's only with
NSTEP_FOLD_KERNEL = "phx_nstep_fold_kernel"              #  `acted`, the gather's only with nstep_next_obs)
NSTEP_GATHER_KERNEL = "phx_nstep_gather_kernel"
NSTEP_MAX_N = 64
EPISODE_SCAN_KERNEL = "phx_episode_scan_kernel"          # (phx_episode_stats: the scan's name, with `summary` joined by "+" with the
EPISODE_REDUCE_KERNEL = "phx_episode_reduce_kernel"      #  reduction's)
BATCH_COUNT_KERNEL = "phx_batch_count_kernel"            # (phx_train_batch: the names of the kernels launched joined by "+"; the moments'
BATCH_SCAN_KERNEL = "phx_batch_scan_kernel"              #  only with std_plane, the scatter's missing where it has nothing to write)
BATCH_MOMENTS_KERNEL = "phx_batch_moments_kernel"
BATCH_SCATTER_KERNEL = "phx_batch_scatter_kernel"
BATCH_KERNELS = "+".join((BATCH_COUNT_KERNEL, BATCH_SCAN_KERNEL, BATCH_MOMENTS_KERNEL, BATCH_SCATTER_KERNEL))
SEQ_COUNT_KERNEL = "phx_seq_count_kernel"                # (phx_seq_batch: as phx_train_batch's, the scatter's also missing where the three
SEQ_SCAN_KERNEL = "phx_seq_scan_kernel"                  #  per-sequence outputs are not given either)
SEQ_MOMENTS_KERNEL = "phx_seq_moments_kernel"
SEQ_SCATTER_KERNEL = "phx_seq_scatter_kernel"
SEQ_KERNELS = "+".join((SEQ_COUNT_KERNEL, SEQ_SCAN_KERNEL, SEQ_MOMENTS_KERNEL, SEQ_SCATTER_KERNEL))
REPLAY_ADD_KERNEL = "phx_replay_add_kernel"              # (phx_replay_add: the copy, then the one-thread commit of the state)
REPLAY_COMMIT_KERNEL = "phx_replay_commit_kernel"
REPLAY_ADD_KERNELS = "+".join((REPLAY_ADD_KERNEL, REPLAY_COMMIT_KERNEL))
REPLAY_SAMPLE_KERNEL = "phx_replay_sample_kernel"
PRIO_FILL_KERNEL = "phx_prio_fill_kernel"                # (phx_prio_add / phx_prio_update: the names joined by "+"; the span's and the path's,
PRIO_SPAN_KERNEL = "phx_prio_span_kernel"                #  one launch per level of more than 256 nodes, are missing for C <= 4096:
PRIO_ZERO_KERNEL = "phx_prio_zero_kernel"                #  prio_kernels(names, C))
PRIO_RAISE_KERNEL = "phx_prio_raise_kernel"
PRIO_PATH_KERNEL = "phx_prio_path_kernel"
PRIO_TOP_KERNEL = "phx_prio_top_kernel"
PRIO_ADD_KERNELS = "+".join((PRIO_FILL_KERNEL, PRIO_SPAN_KERNEL, PRIO_TOP_KERNEL))
PRIO_UPDATE_KERNELS = "+".join((PRIO_ZERO_KERNEL, PRIO_RAISE_KERNEL, PRIO_PATH_KERNEL, PRIO_TOP_KERNEL))
PRIO_SAMPLE_KERNEL = "phx_prio_sample_kernel"
FILTER_SUM_KERNEL = "phx_filter_sum_kernel"              # (phx_filter_update: the five names joined by "+")
FILTER_MEAN_KERNEL = "phx_filter_mean_kernel"
FILTER_CENTER_KERNEL = "phx_filter_center_kernel"
FILTER_M2_KERNEL = "phx_filter_m2_kernel"
FILTER_MERGE_KERNEL = "phx_filter_merge_kernel"
FILTER_UPDATE_KERNELS = "+".join((FILTER_SUM_KERNEL, FILTER_MEAN_KERNEL, FILTER_CENTER_KERNEL, FILTER_M2_KERNEL, FILTER_MERGE_KERNEL))
FILTER_APPLY_KERNEL = "phx_filter_apply_kernel"
MAX_FRAGMENTS = 8


def prio_kernels(names, capacity):
    """what phx_last_kernel() reads after a phx_prio_add / phx_prio_update call on a tree of ``capacity`` slots: ``PRIO_ADD_KERNELS`` /
    ``PRIO_UPDATE_KERNELS`` without the per-level kernel where no level has more than 256 nodes"""
    sparse = capacity > PRIO_FANOUT * PRIO_TOP_NODES
    return "+".join(k for k in names.split("+") if sparse or k not in (PRIO_SPAN_KERNEL, PRIO_PATH_KERNEL))
RH_ACTIONS_IN_DOMAIN, RH_EXO_IN_DOMAIN = 2, 4      # phx_rollout_io.hints


assert C.sizeof(PhxMsgRec) == 16
assert C.sizeof(PhxVtraceIO) == 112      # (stated in include/phantom_amd_vtrace.h)
assert C.sizeof(PhxTrajNextIO) == 96     # (stated in include/phantom_amd_traj.h)
assert C.sizeof(PhxCompactPlane) == 24 and C.sizeof(PhxTrajCompactIO) == 440      # (stated in include/phantom_amd_compact.h)
assert C.sizeof(PhxNstepIO) == 136 and PhxNstepIO.reward.offset == 24 and PhxNstepIO.succ_row.offset == 72      # (stated in include/phantom_amd_nstep.h)
assert PhxNstepIO.n.offset == 16 and PhxNstepIO.gamma.offset == 20 and PhxNstepIO.nstep_next_obs.offset == 128
assert C.sizeof(PhxEpisodeStats) == EPISODE_STATS_BYTES == 48      # (stated in include/phantom_amd_episodes.h, as is every offset below)
assert [getattr(PhxEpisodeStats, n).offset for n, _ in PhxEpisodeStats._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
assert C.sizeof(PhxEpisodeIO) == 112
assert [getattr(PhxEpisodeIO, n).offset for n, _ in PhxEpisodeIO._fields_] == [0, 4, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104]
assert C.sizeof(PhxBatchPlane) == 16 and C.sizeof(PhxBatchMoments) == BATCH_MOMENTS_BYTES == 32      # (stated in include/phantom_amd_batch.h)
assert C.sizeof(PhxTrainBatchIO) == 656
assert [getattr(PhxTrainBatchIO, n).offset for n, _ in PhxTrainBatchIO._fields_] == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 56, 64, 72, 80, 88, 96,
                                                                                     104, 112, 120, 128, 144]
assert [getattr(PhxBatchMoments, n).offset for n, _ in PhxBatchMoments._fields_] == [0, 8, 16, 24, 28]
assert C.sizeof(PhxSeqBatchIO) == 704                    # (stated in include/phantom_amd_seq.h)
assert [getattr(PhxSeqBatchIO, n).offset for n, _ in PhxSeqBatchIO._fields_] == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 56, 64, 72, 80, 88, 96, 104,
                                                                                 112, 120, 128, 136, 144, 152, 160, 168, 176, 192]
assert C.sizeof(PhxReplayState) == REPLAY_STATE_BYTES == 32      # (stated in include/phantom_amd_replay.h, as is every offset below)
assert C.sizeof(PhxReplayAddIO) == 80 and C.sizeof(PhxReplaySampleIO) == 96
assert [getattr(PhxReplayAddIO, n).offset for n, _ in PhxReplayAddIO._fields_] == [0, 8, 16, 24, 28, 32, 40, 48, 56, 64]
assert [getattr(PhxReplaySampleIO, n).offset for n, _ in PhxReplaySampleIO._fields_] == [0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80]
assert C.sizeof(PhxPrioState) == PRIO_STATE_BYTES == 32          # (stated in include/phantom_amd_prio.h, as is every offset below)
assert [getattr(PhxPrioState, n).offset for n, _ in PhxPrioState._fields_] == [0, 4, 8, 16, 24]
assert C.sizeof(PhxPrioAddIO) == 72 and C.sizeof(PhxPrioUpdateIO) == 72 and C.sizeof(PhxPrioSampleIO) == 80
assert [getattr(PhxPrioAddIO, n).offset for n, _ in PhxPrioAddIO._fields_] == [0, 8, 16, 24, 32, 40, 48, 56]
assert [getattr(PhxPrioUpdateIO, n).offset for n, _ in PhxPrioUpdateIO._fields_] == [0, 8, 16, 24, 32, 40, 48, 56]
assert [getattr(PhxPrioSampleIO, n).offset for n, _ in PhxPrioSampleIO._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64]
assert C.sizeof(PhxFilterState) == FILTER_STATE_BYTES == 272      # (stated in include/phantom_amd_filter.h, as is every offset below)
assert [getattr(PhxFilterState, n).offset for n, _ in PhxFilterState._fields_] == [0, 8, 16, 144]
assert C.sizeof(PhxFilterUpdateIO) == 80 and C.sizeof(PhxFilterApplyIO) == 80
assert [getattr(PhxFilterUpdateIO, n).offset for n, _ in PhxFilterUpdateIO._fields_] == [0, 4, 8, 16, 20, 24, 32, 40, 48, 56, 64]
assert [getattr(PhxFilterApplyIO, n).offset for n, _ in PhxFilterApplyIO._fields_] == [0, 4, 8, 16, 20, 24, 32, 40, 48, 56, 64]

_LIB = None
LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")
# PHX_LIB_PATH: development override (A/B runs of experimental builds); the default is the in-tree library
LIB_PATH = os.environ.get("PHX_LIB_PATH") or os.path.join(LIB_DIR, "libphantom_amd.so")

EXPORTS = ("phx_abi_version", "phx_last_error", "phx_last_kernel", "phx_autotune_note", "phx_state_nbytes", "phx_obs_dim",
           "phx_n_strategic", "phx_n_exo", "phx_create", "phx_destroy", "phx_n_fields",
           "phx_field_info", "phx_uses_fused", "phx_sync_fields", "phx_reset", "phx_step", "phx_step_begin", "phx_step_end", "phx_inject",
           "phx_resolve", "phx_rollout", "phx_get_state", "phx_set_state", "phx_trace",
           "phx_pack_flags", "phx_unpack_flags", "phx_mt_seed", "phx_mt_draw")


def built_archs():
    """offload architectures the in-tree library was compiled for (phantom_amd/build.py)."""
    try:
        return [a for a in open(os.path.join(LIB_DIR, "ARCH")).read().strip().split(";") if a]
    except OSError:
        return ["gfx950"]


def _check_arch(torch):
    """Fail at load time, not at the first launch ('invalid device function'), when the visible
    GPU is not one the library holds a code object for."""
    if not torch.cuda.is_available():
        return                         # symbol / spec-size calls work without a GPU; DeviceEnv raises
    name = getattr(torch.cuda.get_device_properties(torch.cuda.current_device()), "gcnArchName", "")
    arch = name.split(":")[0]
    if arch and arch not in built_archs():
        raise RuntimeError(
            f"libphantom_amd.so was built for {built_archs()} but the visible GPU is {arch}: rebuild with "
            f"PHX_OFFLOAD_ARCH='{arch}' (the kernels are tuned for gfx950 / MI355X only)")


def bind_signatures(lib):
    """restype / argtypes of every entry point of include/phantom_amd.h on a loaded library (the ctypes stub of
    INTEGRATION.md section 2).  Used for libphantom_amd.so here and, unchanged, for the CPU restatement behind the same
    symbols in tests (oracle/libphantom_cpu.so: host pointers)."""
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.phx_abi_version.restype = i32
    lib.phx_last_kernel.restype = C.c_char_p
    lib.phx_autotune_note.restype = C.c_char_p
    lib.phx_autotune_note.argtypes = [C.c_void_p]
    lib.phx_last_error.restype = C.c_char_p
    lib.phx_state_nbytes.restype = i64
    lib.phx_state_nbytes.argtypes = [C.POINTER(PhxSpec)]
    for n in ("phx_obs_dim", "phx_n_strategic", "phx_n_exo"):
        getattr(lib, n).restype = i32
        getattr(lib, n).argtypes = [C.POINTER(PhxSpec)]
    lib.phx_create.restype = i32
    lib.phx_create.argtypes = [C.POINTER(PhxSpec), i32, vp, i64, C.POINTER(vp)]
    lib.phx_destroy.restype = None
    lib.phx_destroy.argtypes = [vp]
    lib.phx_n_fields.restype = i32
    lib.phx_n_fields.argtypes = [vp]
    lib.phx_field_info.restype = i32
    lib.phx_field_info.argtypes = [vp, i32, C.POINTER(PhxField)]
    lib.phx_uses_fused.restype = i32
    lib.phx_uses_fused.argtypes = [vp]
    lib.phx_sync_fields.restype = i32
    lib.phx_sync_fields.argtypes = [vp, vp]
    lib.phx_reset.restype = i32
    lib.phx_reset.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    for n in ("phx_step", "phx_step_begin", "phx_step_end"):
        getattr(lib, n).restype = i32
        getattr(lib, n).argtypes = [vp, C.POINTER(PhxStepIO), vp]
    lib.phx_inject.restype = i32
    lib.phx_inject.argtypes = [vp, C.POINTER(PhxMsgRec), i32]
    lib.phx_resolve.restype = i32
    lib.phx_resolve.argtypes = [vp, vp, vp, vp, vp]
    lib.phx_rollout.restype = i32
    lib.phx_rollout.argtypes = [vp, C.POINTER(PhxRolloutIO), vp]
    lib.phx_get_state.restype = i64
    lib.phx_get_state.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.phx_set_state.restype = i64
    lib.phx_set_state.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.phx_trace.restype = i32
    lib.phx_trace.argtypes = [vp, vp, vp, i32, C.POINTER(PhxMsgRec), i32, vp]
    lib.phx_pack_flags.restype = i32
    lib.phx_pack_flags.argtypes = [vp, vp, i64, vp]
    lib.phx_unpack_flags.restype = i32
    lib.phx_unpack_flags.argtypes = [vp, vp, i64, vp]
    lib.phx_mt_seed.restype = i32
    lib.phx_mt_seed.argtypes = [vp, vp, vp]
    lib.phx_mt_draw.restype = i32
    lib.phx_mt_draw.argtypes = [vp, vp, i32, vp]
    return lib


# the learner-side entry points over fragments: each takes (its io struct *, stream) and returns a status (FragmentOps._launch)
FRAGMENT_OPS = {"phx_gae": PhxGaeIO, "phx_gae_masked": PhxGaeMaskedIO, "phx_vtrace": PhxVtraceIO, "phx_traj_next": PhxTrajNextIO,
                "phx_traj_compact": PhxTrajCompactIO, "phx_nstep": PhxNstepIO, "phx_episode_stats": PhxEpisodeIO,
                "phx_train_batch": PhxTrainBatchIO, "phx_seq_batch": PhxSeqBatchIO, "phx_replay_add": PhxReplayAddIO,
                "phx_replay_sample": PhxReplaySampleIO}


# the entry points of include/phantom_amd_prio.h: the same calling convention, a table of their own
PRIORITY_OPS = {"phx_prio_add": PhxPrioAddIO, "phx_prio_update": PhxPrioUpdateIO, "phx_prio_sample": PhxPrioSampleIO}


# the entry points of include/phantom_amd_filter.h: the same calling convention, a table of their own
FILTER_OPS = {"phx_filter_update": PhxFilterUpdateIO, "phx_filter_apply": PhxFilterApplyIO}


def bind_fragment_ops(lib):
    """restype / argtypes of the entry points of include/phantom_amd_{gae,vtrace,traj,compact,nstep,episodes,batch,seq,replay,prio,filter}.h:
    libphantom_amd.so only (the CPU restatement behind phantom_amd.h's symbols has no such functions, so this is not part of
    bind_signatures)"""
    for entry, io in {**FRAGMENT_OPS, **PRIORITY_OPS, **FILTER_OPS}.items():
        getattr(lib, entry).restype = C.c_int32
        getattr(lib, entry).argtypes = [C.POINTER(io), C.c_void_p]
    return lib


def load_library():
    """Load libphantom_amd.so (built in-tree by ``phantom_amd.build``); never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback).")
    # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Import it FIRST so that this
    # library's NEEDED libamdhip64.so.7 resolves to the already-loaded runtime: two HIP runtimes
    # in one process do not share devices/streams ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    bind_signatures(lib)
    bind_fragment_ops(lib)
    if lib.phx_abi_version() != ABI_VERSION:
        raise RuntimeError("libphantom_amd.so ABI version mismatch")
    _check_arch(torch)
    _LIB = lib
    return lib
