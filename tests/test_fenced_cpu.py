"""tests/fenced.py can fail: the checker behind tests/test_gpu_fences.py on CPU tensors -- a byte flipped right before and right
behind a plane, an element left at the poison value, the mask, the planes' alignment and adjacency."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fenced import POISON, assert_fences, assert_poison, assert_written, fenced, fenced_trajectory, poison_word

CPU = torch.device("cpu")
# trailing shapes whose rows are 1, 3, 9 and 549 bytes long (u8), and the f32 / f64 / i32 planes of the GPU module
ROWS = [((1,), torch.uint8), ((3,), torch.uint8), ((9,), torch.uint8), ((61, 9), torch.uint8), ((7, 9), torch.uint8),
        ((5, 3, 3), torch.float32), ((7, 9), torch.float64), ((), torch.uint8), ((), torch.int32), ((5,), torch.int32)]


def _raw(whole):
    return whole.reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("tail,dtype", ROWS, ids=[f"{d}".split(".")[1] + "x".join(map(str, t)) for t, d in ROWS])
@pytest.mark.parametrize("n0", [1, 7, 41])
def test_planes_are_aligned_exact_and_directly_between_their_guards(tail, dtype, n0):
    shape = (n0,) + tail
    plane, whole = fenced(shape, dtype, CPU)
    assert tuple(plane.shape) == shape and plane.dtype == dtype and plane.is_contiguous()
    assert plane.data_ptr() % 16 == 0
    g = (whole.shape[0] - n0) // 2
    assert g >= 16 and g % 16 == 0 and whole.shape[0] == n0 + 2 * g
    raw = _raw(whole)
    nb = plane.numel() * plane.element_size()
    assert raw.numel() == nb + 2 * (plane.data_ptr() - whole.data_ptr())        # guard | plane | guard, nothing else
    assert plane.data_ptr() + nb + g * (nb // n0) == whole.data_ptr() + raw.numel()
    assert (raw == POISON).all()
    assert_fences(whole, n0, "fresh")
    assert_poison(plane, "fresh")
    with pytest.raises(AssertionError, match="not written"):
        assert_written(plane, "fresh")


def test_row_sizes_1_3_9_and_549_bytes():
    for tail, want in (((1,), 1), ((3,), 3), ((9,), 9), ((61, 9), 549)):
        plane, whole = fenced((5,) + tail, torch.uint8, CPU)
        assert plane[0].numel() == want and plane.data_ptr() % 16 == 0
        assert plane.data_ptr() - whole.data_ptr() == 16 * want


@pytest.mark.parametrize("tail,dtype", ROWS[:7], ids=range(7))
def test_one_byte_flipped_just_outside_the_plane_is_reported(tail, dtype):
    shape = (7,) + tail
    for side, off in (("before", -1), ("after", 0)):
        plane, whole = fenced(shape, dtype, CPU)
        plane.zero_()
        assert_fences(whole, 7, "clean")
        start = plane.data_ptr() - whole.data_ptr()
        at = start - 1 if side == "before" else start + plane.numel() * plane.element_size()
        _raw(whole)[at] = 0
        with pytest.raises(AssertionError) as e:
            assert_fences(whole, 7, "the plane's name")
        msg = str(e.value)
        assert "the plane's name" in msg and f"written {side} the plane" in msg and msg.startswith("the plane's name: 1 byte(s)")
        assert f"offsets {off} .. {off} " in msg, msg


def test_the_far_end_of_a_guard_and_the_dirty_range_are_reported():
    plane, whole = fenced((4, 9), torch.uint8, CPU)
    raw = _raw(whole)
    raw[0] = 1
    with pytest.raises(AssertionError, match=r"1 byte\(s\) written before the plane, offsets -144 .. -144 "):
        assert_fences(whole, 4, "p")
    raw[0] = POISON
    raw[-1] = 1; raw[16 * 9 + 36 + 3] = 2
    with pytest.raises(AssertionError, match=r"2 byte\(s\) written after the plane, offsets 3 .. 143 "):
        assert_fences(whole, 4, "p")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.int32, torch.float64])
def test_one_element_left_at_the_poison_value_is_reported_and_the_mask_exempts_it(dtype):
    plane, whole = fenced((6, 5, 3), dtype, CPU)
    plane.fill_(1)
    assert_written(plane, "full")
    raw = plane.reshape(-1).view(torch.uint8)
    es = plane.element_size()
    k = (2 * 15 + 4 * 3 + 1) * es                                  # element [2, 4, 1]
    raw[k:k + es] = POISON
    assert plane.cpu().numpy().view(f"u{es}")[2, 4, 1] == poison_word(es)
    with pytest.raises(AssertionError, match=r"p: 1 of 90 element\(s\) were not written.*first at \(2, 4, 1\)"):
        assert_written(plane, "p")
    mask = np.zeros((6, 5, 3), bool); mask[2, 4, 1] = True
    assert_written(plane, "p", mask)
    lead = np.zeros((6, 5), bool); lead[2, 4] = True               # a mask over the leading dimensions (obs_valid for observations)
    assert_written(plane, "p", lead)
    lead[2, 4] = False; lead[2, 3] = True
    with pytest.raises(AssertionError):
        assert_written(plane, "p", lead)
    if es > 1:                                                     # a partly written element is written
        raw[k] = 0
        assert_written(plane, "p")
    assert_fences(whole, 6, "p")


def test_f32_and_f64_poison_values_are_no_value_an_env_emits():
    assert np.uint32(poison_word(4)).view(np.float32) == np.float32(-2.8735182e-16)
    assert -2.6e-127 < np.uint64(poison_word(8)).view(np.float64) < -2.4e-127
    assert np.uint32(poison_word(4)).view(np.int32) == -1515870811


def _fake_dev(B, S, D, fsm, trace_cap=0):
    return types.SimpleNamespace(B=B, S=S, D=D, device=CPU, spec=types.SimpleNamespace(trace_cap=trace_cap), _needs_valid_planes=lambda: fsm)


def test_fenced_trajectory_has_alloc_trajectorys_planes_and_its_check_fails_on_each_kind_of_mistake():
    T, B, S, D = 5, 7, 9, 3
    tr, wholes, check = fenced_trajectory(_fake_dev(B, S, D, True, 4), T, explore=True, record_messages=True)
    assert tr.observations.shape == (T, B, S, D) and tr.last_obs.shape == (B, S, D) and tr.obs_valid.shape == (T, B, S)
    assert tr.msg_log.shape == (T, B, 4, 16) and tr.msg_count.shape == (T, B) and tr.dist_inputs.shape == (T, B, S, 2)
    assert set(wholes) == {"observations", "actions", "rewards", "truncations", "terminations", "last_obs", "obs_valid", "reward_valid",
                           "msg_log", "msg_count", "raw_actions", "action_logp", "dist_inputs"}
    for p in tr:
        if isinstance(p, torch.Tensor):
            p.zero_()
    check()
    with pytest.raises(AssertionError, match="last_obs"):
        check(last_obs=False)
    tr.rewards[3, 2, 1:3] = torch.tensor(np.array([poison_word(4)] * 2, np.uint32).view(np.float32))
    with pytest.raises(AssertionError, match="rewards: 2 of"):
        check()
    m = np.zeros((T, B, S), bool); m[3, 2, 1:3] = True
    check(masks={"rewards": m})
    with pytest.raises(AssertionError, match="rows 3 .. 4"):
        check(rows=3)
    _raw(wholes["obs_valid"][0])[16 * B * S + T * B * S] = 1
    with pytest.raises(AssertionError, match="obs_valid: 1 byte.s. written after the plane, offsets 0 .. 0 "):
        check(masks={"rewards": m})
    # rows past the fragment's end stay untouched; no terminations plane; no validity planes on a plain env
    tr, wholes, check = fenced_trajectory(_fake_dev(B, S, D, False), T, terminations=False)
    assert tr.terminations is None and tr.obs_valid is None and "terminations" not in wholes
    for p in tr:
        if isinstance(p, torch.Tensor):
            p[:3].zero_()
    tr.last_obs.zero_()
    check(rows=3)
    with pytest.raises(AssertionError, match="not written"):
        check()


def test_joined_flag_planes_are_one_fenced_block():
    T, B, S = 4, 16, 4                                             # T B S = 256
    tr, wholes, check = fenced_trajectory(_fake_dev(B, S, 3, False), T, joined_flags=True)
    assert tr.terminations.data_ptr() == tr.truncations.data_ptr() + T * B * S        # one fill of 2 T B S bytes covers both
    assert "flags" in wholes and "truncations" not in wholes and wholes["flags"][0].shape == (4, T, B, S)
    for p in tr:
        if isinstance(p, torch.Tensor):
            p.zero_()
    check()
    _raw(wholes["flags"][0])[256 + 2 * 256] = 0
    with pytest.raises(AssertionError, match="flags: 1 byte.s. written after"):
        check()
