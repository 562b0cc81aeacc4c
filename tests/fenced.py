"""Fenced, poisoned output buffers for the GPU tests: a kernel that stores one byte outside a plane, or leaves one element of
it unwritten, fails the test.  TEST INFRASTRUCTURE ONLY (no fixture is registered here; works on CPU tensors too).

``torch.empty`` hides both mistakes: the caching allocator rounds every allocation up (a store past a plane's last row lands
in slack nobody reads) and returns whatever the block held before (often the previous call's rows of the same shape).  Here a
plane lies between two guards inside ONE allocation, every byte of which is POISON (0xA5) before the call:

* ``fenced`` carves the plane out so that its first byte directly follows the leading guard and its last byte is directly
  followed by the trailing guard -- no padding, no slack -- and it still starts on a 16-byte boundary;
* ``assert_fences``: both guards are untouched;
* ``assert_written``: no element of the plane still reads as the poison word.
"""
import math

import numpy as np
import torch

POISON = 0xA5
_WORD = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def poison_word(itemsize):
    """the poison as one element of ``itemsize`` bytes reads it: 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5"""
    return _WORD[itemsize](int.from_bytes(bytes([POISON]) * itemsize, "little"))


def _row_bytes(shape, dtype):
    return math.prod(shape[1:]) * torch.empty(0, dtype=dtype).element_size()


def _guard(shape, dtype, guard_rows):
    """guard rows (elements of a 1-D buffer) on each side: ``guard_rows``, or the first multiple of it whose byte count is a
    multiple of 16 (16 rows are, whatever the row size)"""
    g, rb = guard_rows, _row_bytes(shape, dtype)
    while (g * rb) % 16:
        g += guard_rows
    return g


def fenced(shape, dtype, device, guard_rows=16):
    """``(plane, whole)``: ``whole`` has ``g + shape[0] + g`` leading rows (g = guard_rows, see _guard), every byte POISON;
    ``plane = whole[g : g + shape[0]]`` is contiguous, has exactly ``shape`` and starts on a 16-byte boundary."""
    shape = tuple(int(n) for n in shape)
    g, rb = _guard(shape, dtype, guard_rows), _row_bytes(shape, dtype)
    raw = torch.full(((2 * g + shape[0]) * rb,), POISON, dtype=torch.uint8, device=device)
    whole = raw.view(dtype).view((2 * g + shape[0],) + shape[1:])
    plane = whole[g:g + shape[0]]
    assert plane.is_contiguous() and tuple(plane.shape) == shape and plane.data_ptr() % 16 == 0
    return plane, whole


def repoison(whole):
    """every byte of ``whole`` back to POISON (before the next call into the same buffers)"""
    whole.reshape(-1).view(torch.uint8).fill_(POISON)


def _bytes(x):
    """the bytes of a contiguous tensor, on the host"""
    return x.reshape(-1).view(torch.uint8).cpu().numpy()


def assert_fences(whole, shape0, what):
    """every byte of both guards of ``whole`` (from ``fenced``; ``shape0``: the plane's leading rows) is still POISON.  The
    message names the plane, the side, the first and last dirty byte's offset from the plane's edge (before: -1 is the byte
    right in front of the plane; after: 0 is the byte right behind it) and how many bytes are dirty."""
    g = (whole.shape[0] - shape0) // 2
    assert whole.shape[0] == shape0 + 2 * g and g > 0, f"{what}: not a fenced buffer of {shape0} rows"
    b = _bytes(whole)
    n = g * (b.size // whole.shape[0])
    for side, guard, edge in (("before", b[:n], n), ("after", b[b.size - n:], 0)):
        dirty = np.flatnonzero(guard != POISON)
        if dirty.size:
            raise AssertionError(f"{what}: {dirty.size} byte(s) written {side} the plane, offsets {int(dirty[0]) - edge} .. "
                                 f"{int(dirty[-1]) - edge} from its edge (first value 0x{int(guard[dirty[0]]):02x})")


def _words(plane):
    a = plane.contiguous().cpu().numpy()
    return a.view(_WORD[a.dtype.itemsize])


def assert_written(plane, what, mask=None):
    """no element of ``plane`` still holds the poison word: 0xA5 (u8), 0xA5A5A5A5 (f32 / i32), 0xA5A5A5A5A5A5A5A5 (f64 / i64).
    0xA5 is no legal value of a u8 flag or validity plane (0 / 1 / 2); as f32 the word reads as about -2.9e-16 and as f64 as
    about -2.5e-127: no observation (multiples of small integers / 100, prices in [0, 1]), reward or action of these envs takes
    either value, and no int32 output (error codes, message counts) is -1515870811.
    ``mask`` (bool, the plane's shape or its leading dimensions): True EXEMPTS an element the ABI leaves unspecified --
    observations where obs_valid == 0, rewards where reward_valid != 1 on FSM / Stackelberg / ads envs."""
    w = _words(plane)
    left = w == poison_word(w.dtype.itemsize)
    if mask is not None:
        m = np.asarray(mask, bool)
        left &= ~m.reshape(m.shape + (1,) * (left.ndim - m.ndim))
    if left.any():
        idx = np.argwhere(left)
        raise AssertionError(f"{what}: {idx.shape[0]} of {left.size} element(s) were not written (still poison), "
                             f"first at {tuple(int(i) for i in idx[0])}, last at {tuple(int(i) for i in idx[-1])}")


def assert_poison(x, what):
    """every byte of ``x`` is still POISON (rows the call must not touch)"""
    b = _bytes(x.contiguous())
    dirty = np.flatnonzero(b != POISON)
    assert dirty.size == 0, f"{what}: {dirty.size} byte(s) written where nothing may be, byte offsets {int(dirty[0])} .. {int(dirty[-1])}"


def fenced_trajectory(dev, T, terminations=True, explore=False, record_messages=False, joined_flags=False, guard_rows=16):
    """``DeviceEnv.alloc_trajectory(T, ...)`` with every plane fenced and poisoned (``last_obs`` and the validity planes
    included): ``(trajectory, wholes, check)``.  ``wholes[name] = (whole, rows)``.
    ``joined_flags``: ``truncations`` and ``terminations`` are the two halves of ONE fenced ``[2][T][B][S]`` block, as
    alloc_trajectory lays them out when ``(T * B * S) % 256 == 0`` (one zero fill of the library then covers both); the block is
    ``wholes["flags"]``, with one guard row -- a whole plane's size -- on each side.
    ``check(rows=T, masks=None, last_obs=True)``: all fences are intact; rows ``[0, rows)`` of every plane are written, except
    where ``masks[name]`` exempts elements (assert_written); rows ``[rows, T)`` still hold the poison; ``last_obs`` is written
    (True) or untouched (False)."""
    from phantom_amd.device import Trajectory
    B, S, D = dev.B, dev.S, dev.D
    u8, f32, i32 = torch.uint8, torch.float32, torch.int32
    planes, wholes = {}, {}

    def add(name, shape, dtype):
        planes[name], w = fenced(shape, dtype, dev.device, guard_rows)
        wholes[name] = (w, shape[0])

    add("observations", (T, B, S, D), f32); add("actions", (T, B, S), f32); add("rewards", (T, B, S), f32)
    if joined_flags:
        assert terminations, "joined flag planes: both planes"
        assert (T * B * S) % 16 == 0, "joined flag planes: the second plane must start on a 16-byte boundary"
        flags, w = fenced((2, T, B, S), u8, dev.device, 1)       # (a row of the block is a whole plane: one of them on each side)
        wholes["flags"] = (w, 2)
        planes["truncations"], planes["terminations"] = flags[0], flags[1]
    else:
        add("truncations", (T, B, S), u8)
        if terminations:
            add("terminations", (T, B, S), u8)
    add("last_obs", (B, S, D), f32)
    if dev._needs_valid_planes():
        add("obs_valid", (T, B, S), u8); add("reward_valid", (T, B, S), u8)
    if record_messages:
        add("msg_log", (T, B, dev.spec.trace_cap, 16), u8); add("msg_count", (T, B), i32)
    if explore:
        add("raw_actions", (T, B, S), f32); add("action_logp", (T, B, S), f32); add("dist_inputs", (T, B, S, 2), f32)
    tr = Trajectory(**{"terminations": None, **planes})

    def check(rows=T, masks=None, last_obs=True, what=""):
        masks = masks or {}
        for name, (w, n0) in wholes.items():
            assert_fences(w, n0, f"{what}{name}")
        for name, p in planes.items():
            if p is None:
                continue
            if name == "last_obs":
                (assert_written if last_obs else assert_poison)(p, f"{what}last_obs")
                continue
            m = masks.get(name)
            if name == "msg_log":            # 16-byte records: an unwritten one reads as two poison words (a byte of a record may be 0xA5)
                p = p.view(torch.int64)
            assert_written(p[:rows], f"{what}{name}", None if m is None else np.asarray(m)[:rows])
            if rows < T:
                assert_poison(p[rows:], f"{what}{name} rows {rows} .. {T - 1}")

    return tr, wholes, check
