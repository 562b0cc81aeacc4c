"""The definition of phx_prio_add / phx_prio_update / phx_prio_sample (include/phantom_amd_prio.h) restated with numpy: np.float32 for
every add of a chain (in the defined order), Python integers mod 2^64 for the stream of draws.  ``Tree`` rebuilds every level with array
operations after each call; ``NaiveTree`` does the same one node and one draw at a time with scalars and shares nothing with it but the
layout.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
FANOUT = 16
PRIO_MIN, PRIO_MAX = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
STATE_DTYPE = np.dtype([("max_priority", "<f4"), ("reserved0", "<u4"), ("ignored", "<i8"), ("refused", "<i8"), ("reserved1", "<i8")])
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# ---- cases the CPU and the GPU tests share ----
BAD_PRIORITIES = (float("nan"), 0.0, -1.0, float("inf"), 2.0 ** -50, 2.0 ** 50)
# C = 37, size = 37, leaf s = 1 + s mod 7 (stated in the header): (seed, draw) -> (slots, priorities) of 8 draws
KNOWN = {(0, 0): ([12, 11, 11, 18, 22, 17, 4, 8], [6, 5, 5, 5, 2, 4, 5, 2]), (0, 1): ([19, 11, 34, 6, 13, 10, 6, 9], [6, 5, 7, 7, 7, 4, 7, 3]),
         (1, 0): ([16, 16, 20, 30, 6, 5, 27, 13], [3, 3, 7, 3, 7, 6, 7, 7]),
         (2 ** 64 - 1, 2 ** 64 - 1): ([26, 1, 0, 33, 18, 18, 25, 31], [6, 2, 1, 6, 5, 5, 5, 4])}
# the "no k" fallback.  C = 32: leaf 0 = 3 and leaf 16 = 2^24 + 4, every other leaf 2^-40 (absorbed by both chains), so the root's children
# are 3 and 2^24 + 4 and total = fl(2^24 + 7) = 2^24 + 8 (a tie, to even).  Draw 0 of these streams has x >> 40 = 2^24 - 2 or 2^24 - 1:
# m = 2^24 + 6 < total selects child 1, and m - 3 = 2^24 + 3 rounds (a tie, to even) to 2^24 + 4, child 1's own sum: no k has m < s_k
# there, the last positive child is leaf 31.
FALLBACK_DRAWS = ((0, 283417), (0, 9880918), (0, 19210192))


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def layout(C):
    """``(L, n, off, W, words)``: the levels' node counts n[0..L] and offsets off[0..L], the sum part's words and the buffer's"""
    assert 1 <= C <= 2 ** 30
    n, off = [C], [0]
    while n[-1] != 1:
        w = FANOUT * -(-n[-1] // FANOUT)
        off.append(off[-1] + w)
        n.append(w // FANOUT)
    W = off[-1] + FANOUT
    w0 = FANOUT * -(-C // FANOUT)
    return len(n) - 1, n, off, W, W + (W - w0)


def san(p):
    """NaN, zero and negatives: PRIO_MIN; +inf: PRIO_MAX"""
    p = np.float32(p)
    return min(p, PRIO_MAX) if p >= PRIO_MIN else PRIO_MIN


def uniforms(seed, draw, n):
    """u_i of the header for i = 0 .. n - 1: f32, exact"""
    s0 = mix(mix((seed + G) & M64) ^ draw)
    return np.array([(mix((s0 + (i + 1) * G) & M64) >> 40) for i in range(n)], np.float32) * np.float32(2.0 ** -24)


class _Base:
    def __init__(self, C):
        self.C = C
        self.L, self.n, self.off, self.W, self.words = layout(C)
        self.w0 = FANOUT * -(-C // FANOUT)
        self.buf = np.zeros(self.words, np.float32)
        self.max_priority = np.float32(0.0)                       # as stored: 0 reads as 1
        self.ignored = self.refused = 0

    def moff(self, l):
        """where min level l >= 1 starts"""
        return self.W + self.off[l] - self.w0

    def maxp(self):
        return np.float32(1.0) if self.max_priority == 0 else self.max_priority

    def total(self):
        return self.buf[self.off[self.L]]

    def pmin(self):
        return self.buf[self.moff(self.L)] if self.L else self.buf[0]

    def pmin_index(self):
        return self.moff(self.L) if self.L else 0

    def state(self):
        return np.array((self.max_priority, 0, self.ignored, self.refused, 0), STATE_DTYPE)

    def add_slots(self, K, src_capacity, cursor):
        """the slots phx_prio_add names, or None where the count is refused"""
        if K < 0 or K > src_capacity:
            self.refused += 1
            return None
        return (cursor % self.C + np.arange(max(0, K - self.C), K, dtype=np.int64)) % self.C

    def accepted(self, slots, priorities, size):
        size = min(max(size, 0), self.C)
        acc = [(int(s), san(p)) for s, p in zip(slots, priorities) if 0 <= int(s) < size]
        self.ignored += len(slots) - len(acc)
        if acc:
            self.max_priority = max(self.maxp(), max(p for _, p in acc))
        return acc


class Tree(_Base):
    def rebuild(self):
        b = self.buf
        for l in range(1, self.L + 1):
            c = b[self.off[l - 1]:self.off[l - 1] + FANOUT * self.n[l]].reshape(self.n[l], FANOUT)
            s = c[:, 0].copy()
            for k in range(1, FANOUT):
                s = s + c[:, k]                                    # f32 + f32 -> f32: the chain, in order
            b[self.off[l]:self.off[l] + self.n[l]] = s
            m = c if l == 1 else b[self.moff(l - 1):self.moff(l - 1) + FANOUT * self.n[l]].reshape(self.n[l], FANOUT)
            mn = np.where(m > 0, m, np.float32(np.inf)).min(axis=1)
            b[self.moff(l):self.moff(l) + self.n[l]] = np.where(np.isinf(mn), np.float32(0), mn)

    def add(self, K, src_capacity, cursor):
        p = self.maxp()
        slots = self.add_slots(K, src_capacity, cursor)
        if slots is None:
            return
        self.buf[slots] = p
        self.rebuild()

    def update(self, slots, priorities, size):
        acc = self.accepted(slots, priorities, size)
        if acc:
            s, p = np.array([a[0] for a in acc], np.int64), np.array([a[1] for a in acc], np.float32)
            self.buf[s] = 0
            np.maximum.at(self.buf, s, p)
        self.rebuild()

    def sample(self, n, seed, draw, size):
        """``(out_slot [n] i64, out_priority [n] f32)``"""
        size = min(max(size, 0), self.C)
        total = self.total()
        if total == 0 or size == 0:
            return np.full(n, -1, np.int64), np.zeros(n, np.float32)
        m = uniforms(seed, draw, n) * total
        j = np.zeros(n, np.int64)
        rows = np.arange(n)
        for l in range(self.L, 0, -1):
            c = self.buf[self.off[l - 1] + FANOUT * j[:, None] + np.arange(FANOUT)]
            s = np.empty_like(c)
            s[:, 0] = c[:, 0]
            for k in range(1, FANOUT):
                s[:, k] = s[:, k - 1] + c[:, k]
            below = m[:, None] < s
            pos = c > 0
            last = np.where(pos.any(axis=1), FANOUT - 1 - pos[:, ::-1].argmax(axis=1), 0)
            k = np.where(below.any(axis=1), below.argmax(axis=1), last)
            m = m - np.where(k > 0, s[rows, np.maximum(k - 1, 0)], np.float32(0))
            j = np.minimum(FANOUT * j + k, self.n[l - 1] - 1)
        leaf = self.buf[j]
        ok = (j < size) & (leaf > 0)
        return np.where(ok, j, -1), np.where(ok, leaf, np.float32(0)).astype(np.float32)


class NaiveTree(_Base):
    """every node from the leaves, one scalar add at a time; every draw one scalar descent"""

    def rebuild(self):
        b = self.buf
        b[self.w0:] = 0
        for l in range(1, self.L + 1):
            for j in range(self.n[l]):
                s, mn = None, np.float32(0)
                for k in range(FANOUT):
                    c = np.float32(b[self.off[l - 1] + FANOUT * j + k])
                    s = c if s is None else np.float32(s + c)
                    v = c if l == 1 else np.float32(b[self.moff(l - 1) + FANOUT * j + k])
                    if v != 0 and (mn == 0 or v < mn):
                        mn = v
                b[self.off[l] + j] = s
                b[self.moff(l) + j] = mn

    def add(self, K, src_capacity, cursor):
        p = self.maxp()
        slots = self.add_slots(K, src_capacity, cursor)
        if slots is None:
            return
        for s in slots.tolist():                                   # one leaf after the other
            self.buf[s] = p
        self.rebuild()

    def update(self, slots, priorities, size):
        acc = self.accepted(slots, priorities, size)
        for s in {a[0] for a in acc}:
            self.buf[s] = max(p for t, p in acc if t == s)
        self.rebuild()

    def sample(self, n, seed, draw, size, fallbacks=None):
        """as ``Tree.sample``; ``fallbacks``: a list that receives (draw index, level) wherever no k had m < s_k"""
        size = min(max(size, 0), self.C)
        total = np.float32(self.total())
        out_slot, out_p = np.full(n, -1, np.int64), np.zeros(n, np.float32)
        if total == 0 or size == 0:
            return out_slot, out_p
        for i, u in enumerate(uniforms(seed, draw, n)):
            m, j = np.float32(u * total), 0
            for l in range(self.L, 0, -1):
                s, prev, kstar, base, last, last_base = None, np.float32(0), None, None, 0, np.float32(0)
                for k in range(FANOUT):
                    c = np.float32(self.buf[self.off[l - 1] + FANOUT * j + k])
                    prev = np.float32(0) if s is None else s
                    s = c if s is None else np.float32(s + c)
                    if kstar is None and m < s:
                        kstar, base = k, prev
                    if c > 0:
                        last, last_base = k, prev
                if kstar is None:
                    kstar, base = last, last_base
                    if fallbacks is not None:
                        fallbacks.append((i, l))
                m = np.float32(m - base)
                j = min(FANOUT * j + kstar, self.n[l - 1] - 1)
            leaf = np.float32(self.buf[j])
            if j < size and leaf > 0:
                out_slot[i], out_p[i] = j, leaf
        return out_slot, out_p
