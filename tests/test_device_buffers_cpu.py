"""phantom_amd._buffers on CPU tensors: the byte layouts DeviceEnv puts in one buffer (offsets derived from the rule
"sections in the listed order, each rounded up to 256 bytes") and the argument check in front of every raw pointer."""
import numpy as np
import pytest
import torch

from phantom_amd._buffers import AtLeast, Layout, check_tensor
from phantom_amd.device import _fragment_layout, _step_layout

CPU = torch.device("cpu")


def _offsets(layout):
    return {k: (off, n) for k, (off, n, _, _) in layout.sections.items()}


def test_step_output_layout():
    lay = _step_layout(3, 2, 3)
    assert [off for off, _ in _offsets(lay).values()] == list(range(0, 2560, 256))
    assert list(lay.sections) == ["obs", "reward", "obs_valid", "reward_valid", "terminated", "truncated", "done_valid",
                                  "all_terminated", "all_truncated", "err"]
    assert lay.sections["obs"][:2] == (0, 72) and lay.sections["reward"][:2] == (256, 48) and lay.sections["err"][:2] == (2304, 12)
    assert lay.nbytes == 2560


def test_flat_fragment_layout_plain():
    lay = _fragment_layout(2, 3, 2, 3, valid_planes=False, flag_planes=1)
    assert _offsets(lay) == {"observations": (0, 144), "actions": (256, 48), "rewards": (512, 48), "packed_flags": (768, 8),
                             "truncations": (1024, 12), "terminations": (1280, 12), "last_obs": (1536, 72)}
    assert lay.end("packed_flags") == 1024 and lay.nbytes == 1792
    assert lay.end("last_obs") == lay.nbytes and lay.end("observations") == 256


def test_flat_fragment_layout_valid_planes_two_flag_planes():
    lay = _fragment_layout(2, 3, 2, 3, valid_planes=True, flag_planes=2)
    assert {k: off for k, (off, _) in _offsets(lay).items()} == {
        "observations": 0, "actions": 256, "rewards": 512, "obs_valid": 768, "reward_valid": 1024, "packed_flags": 1280,
        "truncations": 1536, "terminations": 1792, "last_obs": 2048}
    assert lay.sections["packed_flags"][1] == 16
    assert lay.end("packed_flags") == 1536 and lay.nbytes == 2304


def test_a_section_of_a_whole_number_of_lines_is_not_padded():
    lay = Layout([("a", (128,), torch.float32), ("b", (1,), torch.uint8), ("c", (65,), torch.float32)])
    assert _offsets(lay) == {"a": (0, 512), "b": (512, 1), "c": (768, 260)} and lay.nbytes == 1280


def test_views_share_the_buffer():
    lay = Layout([("f", (2, 3), torch.float32), ("d", (3,), torch.float64), ("u", (5,), torch.uint8), ("i", (2,), torch.int32)])
    flat = torch.zeros(lay.nbytes, dtype=torch.uint8)
    tv, nv = lay.torch_views(flat), lay.numpy_views(flat.numpy())
    assert [nv[k].dtype for k in "fdui"] == [np.float32, np.float64, np.uint8, np.int32]
    for k, fill in zip("fdui", (1.5, -2.25, 7, -3)):
        assert tuple(tv[k].shape) == nv[k].shape == lay.sections[k][2]
        tv[k].fill_(fill)
        assert (nv[k] == fill).all()
    inside = np.zeros(lay.nbytes, bool)
    for off, n, _, _ in lay.sections.values():
        inside[off:off + n] = True
    assert inside.sum() == 24 + 24 + 5 + 8 and not flat.numpy()[~inside].any()      # nothing outside the sections was written
    rows = lay.torch_views(torch.zeros((4, lay.nbytes), dtype=torch.uint8))      # leading dimensions are kept
    assert tuple(rows["f"].shape) == (4, 2, 3) and rows["i"].dtype == torch.int32


def test_check_tensor_accepts():
    x = torch.zeros(5, 3, 2)
    check_tensor("t", "x", x, torch.float32, (5, 3, 2), device=CPU)
    check_tensor("t", "x", x, torch.float32, (3, 2), lead=5, device=CPU)
    check_tensor("t", "x", x, torch.float32, (3, 2), lead=AtLeast(4), align=16, device=CPU)
    check_tensor("t", "x", x.to(torch.int16), (torch.int16, torch.uint16), (5, 3, 2), device=CPU)


@pytest.mark.parametrize("case", ["none", "dtype", "transposed", "tail", "rank", "lead_short", "lead_min_short", "lead_long",
                                  "device", "meta", "align"])
def test_check_tensor_refuses(case):
    x = torch.zeros(5, 3, 2)
    kw = dict(dtype=torch.float32, shape=(3, 2), lead=5, device=CPU, align=None)
    if case == "none":
        x = None
    elif case == "dtype":
        x = x.double()
    elif case == "transposed":
        x = torch.zeros(5, 2, 3).transpose(1, 2)
    elif case == "tail":
        kw["shape"] = (3, 3)
    elif case == "rank":
        kw["shape"] = (3, 2, 1)
    elif case == "lead_short":
        kw["lead"] = 6
    elif case == "lead_min_short":
        kw["lead"] = AtLeast(6)
    elif case == "lead_long":
        kw["lead"] = 4
    elif case == "device":
        kw["device"] = torch.device("meta")
    elif case == "meta":
        x = x.to("meta")
    elif case == "align":
        x, kw = torch.zeros(9)[1:], dict(dtype=torch.float32, shape=(8,), lead=None, device=CPU, align=16)
    with pytest.raises(ValueError, match="^rollout: `out.x` "):
        check_tensor("rollout", "out.x", x, kw["dtype"], kw["shape"], lead=kw["lead"], align=kw["align"], device=kw["device"])


def test_check_tensor_alignment_defaults_to_the_element_size():
    x = torch.zeros(9)[1:]                                       # 4 bytes past an allocation's (at least 16-byte aligned) start
    assert x.data_ptr() % 16 == 4
    check_tensor("t", "x", x, torch.float32, (8,), device=CPU)
