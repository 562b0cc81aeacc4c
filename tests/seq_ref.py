"""The definition of phx_seq_batch (include/phantom_amd_seq.h) restated in numpy, twice: ``seq_batch`` vectorised, and ``seq_batch_loop``
as a plain per-element Python loop over columns and rows that follows the header's four steps.  The kept mask, the record layout, the
permutation and the moments are tests/batch_ref.py's.  Sources are u8 ``[T, N]`` (a byte plane) or u32 ``[T, N]`` / ``[T, N, w]`` (bit
patterns); a plane is ``(src, word_off)``.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import batch_ref as br


def _flags(T, N, terminated, truncated):
    f = np.zeros((T, N), bool)
    for x in (terminated, truncated):
        if x is not None:
            f |= np.asarray(x).reshape(T, N) != 0
    return f


def _empty(N):
    return dict(seq_start=np.zeros(N + 1, np.int64), Q=0, K=0, L=0, records=None, out_row=None, out_col=None, seq_lens=None, seq_row=None,
                seq_col=None, moments=None)


def seq_batch(T, N, planes, row_words, L, keep=None, terminated=None, truncated=None, col_class=None, class_id=0, shuffle=1, seed=0, epoch=0,
              std_plane=-1, capacity=None):
    """dict(seq_start, Q, K, L, records u32 [Q * L, row_words], out_row, out_col i32 [Q * L], seq_lens, seq_row, seq_col i32 [Q], moments or
    None); everything but seq_start and moments is None where Q > capacity: the call writes none of it"""
    k = br.kept_mask(T, N, keep, col_class, class_id)
    nn, tt = np.nonzero(k.T)                                      # the kept elements, column by column, t ascending
    E = len(nn)
    f = _flags(T, N, terminated, truncated)[tt, nn]
    e = np.arange(E)
    brk = np.ones(E, bool)                                        # a run of rows that only the length can cut starts here
    brk[1:] = (nn[1:] != nn[:-1]) | f[:-1]
    i = (e - np.maximum.accumulate(np.where(brk, e, 0))) % L      # the position in the sequence
    opens = i == 0
    sid = np.cumsum(opens) - 1
    Q = int(opens.sum())
    res = _empty(N)
    np.cumsum(np.bincount(nn[opens], minlength=N), out=res["seq_start"][1:])
    res.update(Q=Q, K=E, L=L)
    assert res["seq_start"][N] == Q
    if std_plane >= 0:
        x = br._words(planes[std_plane][0])[..., 0].view(np.float32)
        res["moments"] = br.moments_of(x, k)
    if capacity is not None and Q > capacity:
        return res
    sigma = br.perm(Q, seed, epoch, shuffle)
    slot = sigma[sid] * L + i
    rec = np.zeros((Q * L, row_words), np.uint32)
    for p, (src, off) in enumerate(planes):
        w = br._words(src)[tt, nn]
        if p == std_plane:
            with np.errstate(all="ignore"):
                w = ((w.view(np.float32) - res["moments"]["mean"]) / res["moments"]["den"]).astype(np.float32).view(np.uint32)
        rec[slot, off:off + w.shape[1]] = w
    row, col = np.full(Q * L, -1, np.int32), np.full(Q * L, -1, np.int32)
    row[slot], col[slot] = tt, nn
    lens, srow, scol = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    lens[sigma] = np.bincount(sid, minlength=Q)
    srow[sigma], scol[sigma] = tt[opens], nn[opens]
    res.update(records=rec, out_row=row, out_col=col, seq_lens=lens, seq_row=srow, seq_col=scol)
    return res


def seq_batch_loop(T, N, planes, row_words, L, keep=None, terminated=None, truncated=None, col_class=None, class_id=0, shuffle=1, seed=0,
                   epoch=0, std_plane=-1, capacity=None):
    """the same by the header's walk: every column on its own, t ascending, carrying len and g"""
    kp = None if keep is None else np.asarray(keep).reshape(T, N)
    te = None if terminated is None else np.asarray(terminated).reshape(T, N)
    tr = None if truncated is None else np.asarray(truncated).reshape(T, N)
    is_kept = lambda t, n: (kp is None or kp[t, n] != 0) and (col_class is None or col_class[n % len(col_class)] == class_id)
    seqs = []                                                     # per column: [first_row, [kept rows]] per sequence
    for n in range(N):
        mine, ln = [], 0
        for t in range(T):
            if not is_kept(t, n):
                continue
            if ln == 0:
                mine.append([t, []])
            mine[-1][1].append(t)
            ln += 1
            if (te is not None and te[t, n] != 0) or (tr is not None and tr[t, n] != 0) or ln == L:
                ln = 0
        seqs.append(mine)
    res = _empty(N)
    for n in range(N):
        res["seq_start"][n + 1] = res["seq_start"][n] + len(seqs[n])
    Q = int(res["seq_start"][N])
    K = sum(len(rows) for mine in seqs for _, rows in mine)
    res.update(Q=Q, K=K, L=L)
    words = [br._words(src) for src, _ in planes]
    mean = den = None
    if std_plane >= 0:
        one = br.train_batch_loop(T, N, [(planes[std_plane][0], 0)], 4, keep=keep, col_class=col_class, class_id=class_id, std_plane=0, capacity=0)
        res["moments"] = one["moments"]                           # (phantom_amd_batch.h's rule to the letter: its own loop)
        mean, den = one["moments"]["mean"], one["moments"]["den"]
    if capacity is not None and Q > capacity:
        return res
    keys = br.round_keys(seed, epoch)
    rec = np.zeros((Q * L, row_words), np.uint32)
    row, col = np.full(Q * L, -1, np.int32), np.full(Q * L, -1, np.int32)
    lens, srow, scol = np.full(Q, -1, np.int32), np.full(Q, -1, np.int32), np.full(Q, -1, np.int32)
    written = np.zeros(Q * L, bool)
    for n in range(N):
        for g, (first_row, rows) in enumerate(seqs[n]):
            s = int(res["seq_start"][n]) + g
            sigma = br.perm_one(s, Q, keys) if shuffle and Q > 1 else s
            assert lens[sigma] == -1 and 1 <= len(rows) <= L
            lens[sigma], srow[sigma], scol[sigma] = len(rows), first_row, n
            for i in range(L):
                slot = sigma * L + i
                assert not written[slot]
                written[slot] = True
                if i >= len(rows):
                    continue                                      # padding: zeros and -1, as initialised
                t = rows[i]
                row[slot], col[slot] = t, n
                for p, (_, off) in enumerate(planes):
                    for j in range(words[p].shape[2]):
                        u = words[p][t, n, j]
                        if p == std_plane:
                            u = np.float32((np.float32(u.view(np.float32) - mean)) / den).view(np.uint32)
                        rec[slot, off + j] = u
    assert written.all()
    res.update(records=rec, out_row=row, out_col=col, seq_lens=lens, seq_row=srow, seq_col=scol)
    return res


KEYS = ("records", "out_row", "out_col", "seq_lens", "seq_row", "seq_col", "moments")


def same(a, b):
    """two results are equal byte for byte"""
    assert a["Q"] == b["Q"] and a["K"] == b["K"] and a["seq_start"].tobytes() == b["seq_start"].tobytes()
    for k in KEYS:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or (a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()), k
