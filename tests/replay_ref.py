"""The definition of phx_replay_add / phx_replay_sample (include/phantom_amd_replay.h) restated with numpy and Python integers: the
state machine, the slot arithmetic and the draws.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
STATE_DTYPE = np.dtype([("cursor", "<i8"), ("size", "<i8"), ("total", "<i8"), ("refused", "<i8")])


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws(seed, draw, size, n, first=0):
    """the header's s_i for i = first .. first + n - 1 as Python ints: -1 where size == 0"""
    s0 = mix(mix((seed + G) & M64) ^ draw)
    if size == 0:
        return [-1] * n
    return [(mix((s0 + (i + 1) * G) & M64) * size) >> 64 for i in range(first, first + n)]


class Ring:
    """ring [C][row_words] u32 and its state; ``fill``: what the ring's words hold before the first add (the poison of a test)"""

    def __init__(self, C, row_words, fill=0):
        self.C, self.row_words = C, row_words
        self.ring = np.full((C, row_words), fill, np.uint32)
        self.cursor = self.size = self.total = self.refused = 0

    def state(self):
        return np.array((self.cursor, self.size, self.total, self.refused), STATE_DTYPE)

    def add(self, src, K):
        """the header's phx_replay_add with vectorised slot arithmetic"""
        C = self.C
        if K < 0 or K > len(src):
            self.refused += 1
            return
        j = np.arange(max(0, K - C), K, dtype=np.int64)
        self.ring[(self.cursor + j) % C] = src[j]
        self.cursor, self.size, self.total = (self.cursor + K) % C, min(C, self.size + K), self.total + K

    def sample(self, n, seed=0, draw=0, slot_in=None):
        """``(out [n][row_words] u32, out_slot [n] i64)``"""
        if slot_in is None:
            s = np.array(draws(seed, draw, self.size, n), np.int64)
        else:
            s = np.asarray(slot_in, np.int64)
            s = np.where((s >= 0) & (s < self.size), s, -1)
        out = np.where((s >= 0)[:, None], self.ring[np.maximum(s, 0)], np.uint32(0))
        return out.astype(np.uint32), s


class NaiveRing:
    """the same, one record after the other: a deque's behaviour written out, nothing shared with ``Ring.add`` but the field names"""

    def __init__(self, C, row_words, fill=0):
        self.C = C
        self.ring = [[fill] * row_words for _ in range(C)]
        self.cursor = self.size = self.total = self.refused = 0

    def add(self, src, K):
        if K < 0 or K > len(src):
            self.refused += 1
            return
        for j in range(K):                                       # every record in turn: a later one overwrites an earlier one
            self.ring[self.cursor] = [int(x) for x in src[j]]
            self.cursor = self.cursor + 1 if self.cursor + 1 < self.C else 0
            self.size = min(self.C, self.size + 1)
            self.total += 1
