"""phx_train_batch (include/phantom_amd_batch.h) against the same result from the same planes with what the library offered before it,
and against the bytes it needs.
    python tools/batch_time.py [--out profiles/batch_time.txt] [--seconds 0.5] [--repeats 5] [--rows 20 100]
GPU only: no device, no number.  SC64's shape (B = 4 096 env instances, S = 9 agents, D = 3: N = 36 864 columns), T = 20 and 100 rows,
a 5-shop FSM chain's alternating `keep` (the agents act in every other row: K = T N / 2), the 9-column PPO set -- obs and new_obs
(3 words each), actions, rewards, two flag planes (bytes), vf_preds, advantages, value_targets: 13 words in a 16-word record --
advantages standardized, rows shuffled, out_row and out_col written.
The other path: phx_traj_compact into dense arrays, then torch on the device -- the mean and the standard deviation of the kept
advantages and the affine map, torch.randperm(K) and one index_select per column (out_row and out_col included).  It is handed K
(known here, T N / 2) so that it needs no host wait; a caller who must read start[N] first pays that on top.
The tool first checks the call against that path: the records sorted by (column, row) hold the dense arrays bit for bit, the
standardized column within 1e-5.  Then, in ONE process, alternating, `repeats` windows of `seconds` each (HIP events around the
window), buffer sets rotated over more than 256 MB.  Expected bytes per call (each plane read once by the scatter, keep and the
advantages once more by the count): (46 + 1 + 5) T N in, (64 + 8) K out."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
B, S, D = 4096, 9, 3
TS = (20, 100)
COLUMNS = (("obs", D, "f32"), ("new_obs", D, "f32"), ("actions", 1, "f32"), ("rewards", 1, "f32"), ("terminateds", 1, "u8"),
           ("truncateds", 1, "u8"), ("vf_preds", 1, "f32"), ("advantages", 1, "f32"), ("value_targets", 1, "f32"))
ROW_WORDS = 16
TORCH = "phx_traj_compact + torch: moments, randperm, index_select"


def window(fn, seconds, torch):
    """microseconds per call of fn(i) over a window of about `seconds` (HIP events around the whole window)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(0); e1.record(); torch.cuda.synchronize()
    n = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for i in range(n):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def expected_bytes(T, N, K):
    return (46 + 1 + 5) * T * N + (4 * ROW_WORDS + 8) * K


def make_set(torch, _abi, T, N, gen, dev):
    cap = T * N // 2 + N
    planes = {}
    for name, w, kind in COLUMNS:
        shape = (T, N) if w == 1 else (T, N, w)
        planes[name] = (torch.rand(shape, generator=gen, device=dev) < 0.1).to(torch.uint8) if kind == "u8" else \
            3.0 * torch.randn(shape, generator=gen, device=dev) + 1.0
    keep = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    keep[0::2] = 1
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    out = dict(start=e((N + 1,), torch.int64), records=e((cap, ROW_WORDS), torch.int32), out_row=e((cap,), torch.int32), out_col=e((cap,), torch.int32),
               moments=e((32,), torch.uint8), workspace=e((N, 2), torch.float64))
    io = _abi.PhxTrainBatchIO(T=T, N=N, capacity=cap, n_planes=len(COLUMNS), row_words=ROW_WORDS, S=1, class_id=0,
                              std_plane=[c[0] for c in COLUMNS].index("advantages"), shuffle=1, seed=1, epoch=0, keep=keep.data_ptr(),
                              **{k: v.data_ptr() for k, v in out.items()})
    off, layout = 0, {}
    for i, (name, w, kind) in enumerate(COLUMNS):
        io.plane[i] = _abi.PhxBatchPlane(src=planes[name].data_ptr(), elem_bytes=1 if kind == "u8" else 4 * w, word_off=off)
        layout[name] = (off, w)
        off += w
    # the other path's buffers: phx_traj_compact's dense arrays
    dense = {name: e((cap,) + ((w,) if w > 1 else ()), torch.uint8 if kind == "u8" else torch.float32) for name, w, kind in COLUMNS}
    cstart, crow, ccol = e((N + 1,), torch.int64), e((cap,), torch.int32), e((cap,), torch.int32)
    cio = _abi.PhxTrajCompactIO(T=T, n_planes=len(COLUMNS), N=N, capacity=cap, keep=keep.data_ptr(), start=cstart.data_ptr(),
                                out_row=crow.data_ptr(), out_col=ccol.data_ptr())
    for i, (name, w, kind) in enumerate(COLUMNS):
        cio.plane[i] = _abi.PhxCompactPlane(src=planes[name].data_ptr(), dst=dense[name].data_ptr(), elem_bytes=1 if kind == "u8" else 4 * w, reserved=0)
    return dict(planes=planes, keep=keep, out=out, io=io, layout=layout, dense=dense, cio=cio, crow=crow, ccol=ccol)


def in_torch(torch, lib, s, K, stream):
    """the parent's path to the same batch"""
    if lib.phx_traj_compact(C.byref(s["cio"]), stream) != 0:
        raise RuntimeError(lib.phx_last_error().decode())
    adv = s["dense"]["advantages"][:K]
    mean, std = adv.mean(), adv.std(unbiased=False).clamp_min(1e-4)
    perm = torch.randperm(K, device=adv.device)
    res = {name: (x[:K] if name != "advantages" else (adv - mean) / std).index_select(0, perm) for name, x in s["dense"].items()}
    res["row"], res["col"] = s["crow"][:K].index_select(0, perm), s["ccol"][:K].index_select(0, perm)
    return res


def measure(lib, _abi, torch, np, T, seconds, repeats, dev):
    N = B * S
    K = (T + 1) // 2 * N
    gen = torch.Generator(device=dev).manual_seed(0)
    one = expected_bytes(T, N, K)
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets = [make_set(torch, _abi, T, N, gen, dev) for _ in range(n_sets)]
    refs = [C.byref(s["io"]) for s in sets]

    def call(i):
        if lib.phx_train_batch(refs[i % n_sets], stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    calls = {"phx_train_batch": call, TORCH: lambda i: in_torch(torch, lib, sets[i % n_sets], K, stream)}
    s = sets[0]
    call(0)
    in_torch(torch, lib, s, K, stream)
    torch.cuda.synchronize()
    assert int(s["out"]["start"][N]) == K
    rec = s["out"]["records"][:K]
    order = torch.argsort(s["out"]["out_col"][:K].long() * T + s["out"]["out_row"][:K].long())
    ok = True
    for name, w, kind in COLUMNS:
        off = s["layout"][name][0]
        got = rec[order, off:off + w]
        want = s["dense"][name][:K].view(K, w)
        if name == "advantages":
            adv = want[:, 0]
            ref = (adv - adv.mean()) / adv.std(unbiased=False).clamp_min(1e-4)
            ok = ok and bool(((got.view(torch.float32)[:, 0] - ref).abs() <= 1e-5).all())
        else:
            ok = ok and bool((got == (want.to(torch.int32) if kind == "u8" else want.view(torch.int32))).all())
    if not ok:
        raise RuntimeError(f"the call and the torch path disagree (T = {T})")
    for i in range(n_sets):
        call(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds, torch))
    return dict(T=T, N=N, K=K, sets=n_sets, bytes=one, us=us)


SEQ_TORCH = "phx_train_batch(shuffle=0) + torch: chop, pad, randperm"


def make_seq_set(torch, _abi, lib, T, N, L, gen, dev, stream):
    s = make_set(torch, _abi, T, N, gen, dev)
    for name in ("terminateds", "truncateds"):            # an episode end about every 50 kept rows
        s["planes"][name].copy_((torch.rand((T, N), generator=gen, device=dev) < 0.01).to(torch.uint8))
    s["io"].shuffle = 0                                   # the other path's first step: records in (column, row) order
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    start, moments, workspace = e((N + 1,), torch.int64), e((32,), torch.uint8), e((3, N), torch.float64)
    io = _abi.PhxSeqBatchIO(T=T, N=N, capacity=0, n_planes=len(COLUMNS), row_words=ROW_WORDS, S=1, class_id=0,
                            std_plane=[c[0] for c in COLUMNS].index("advantages"), shuffle=1, seed=1, epoch=0, keep=s["keep"].data_ptr(),
                            max_seq_len=L, terminated=s["planes"]["terminateds"].data_ptr(), truncated=s["planes"]["truncateds"].data_ptr(),
                            seq_start=start.data_ptr(), moments=moments.data_ptr(), workspace=workspace.data_ptr())
    for i in range(len(COLUMNS)):
        io.plane[i] = s["io"].plane[i]
    if lib.phx_seq_batch(C.byref(io), stream) != 0:        # capacity 0: the count alone, for Q
        raise RuntimeError(lib.phx_last_error().decode())
    Q = int(start[N])
    out = dict(records=e((Q, L, ROW_WORDS), torch.int32), out_row=e((Q, L), torch.int32), out_col=e((Q, L), torch.int32), seq_lens=e((Q,), torch.int32),
               seq_row=e((Q,), torch.int32), seq_col=e((Q,), torch.int32))
    io.capacity = Q
    for k, v in out.items():
        setattr(io, k, v.data_ptr())
    s.update(seq_io=io, seq_out=out, seq_start=start, Q=Q, seq_moments=moments, seq_workspace=workspace)
    return s


def seq_in_torch(torch, lib, s, K, L, stream):
    """the parent's path to the same sequences"""
    if lib.phx_train_batch(C.byref(s["io"]), stream) != 0:
        raise RuntimeError(lib.phx_last_error().decode())
    Q = s["Q"]
    rec, row, col = s["out"]["records"][:K], s["out"]["out_row"][:K], s["out"]["out_col"][:K]
    flag = (rec[:, s["layout"]["terminateds"][0]] != 0) | (rec[:, s["layout"]["truncateds"][0]] != 0)
    e = torch.arange(K, device=rec.device)
    brk = torch.ones(K, dtype=torch.bool, device=rec.device)
    brk[1:] = (col[1:] != col[:-1]) | flag[:-1]
    i = (e - torch.cummax(torch.where(brk, e, 0), 0).values) % L
    opens = i == 0
    sid = torch.cumsum(opens, 0) - 1
    perm = torch.randperm(Q, device=rec.device)
    sigma = perm.index_select(0, sid)
    slot = sigma * L + i
    records = torch.zeros((Q * L, ROW_WORDS), dtype=torch.int32, device=rec.device).index_copy_(0, slot, rec)
    orow = torch.full((Q * L,), -1, dtype=torch.int32, device=rec.device).index_copy_(0, slot, row)
    ocol = torch.full((Q * L,), -1, dtype=torch.int32, device=rec.device).index_copy_(0, slot, col)
    lens = torch.zeros(Q, dtype=torch.int32, device=rec.device).index_add_(0, sigma, torch.ones((), dtype=torch.int32, device=rec.device).expand(K))
    orow, ocol = orow.view(Q, L), ocol.view(Q, L)
    return dict(records=records.view(Q, L, ROW_WORDS), out_row=orow, out_col=ocol, seq_lens=lens, seq_row=orow[:, 0], seq_col=ocol[:, 0])


def seq_expected_bytes(T, N, Q, L):
    return (46 + 3 + 7) * T * N + (4 * ROW_WORDS + 8) * Q * L + 12 * Q


def measure_seq(lib, _abi, torch, np, T, L, seconds, repeats, dev):
    N = B * S
    K = (T + 1) // 2 * N
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets = [make_seq_set(torch, _abi, lib, T, N, L, gen, dev, stream)]
    one = seq_expected_bytes(T, N, sets[0]["Q"], L)
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    sets += [make_seq_set(torch, _abi, lib, T, N, L, gen, dev, stream) for _ in range(n_sets - 1)]
    refs = [C.byref(s["seq_io"]) for s in sets]

    def call(i):
        if lib.phx_seq_batch(refs[i % n_sets], stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    calls = {"phx_seq_batch": call, SEQ_TORCH: lambda i: seq_in_torch(torch, lib, sets[i % n_sets], K, L, stream)}
    s = sets[0]
    call(0)
    want = seq_in_torch(torch, lib, s, K, L, stream)
    torch.cuda.synchronize()
    Q, got = s["Q"], s["seq_out"]
    assert int(s["seq_start"][N]) == Q and int(s["out"]["start"][N]) == K and int(got["seq_lens"].sum()) == K
    oa = torch.argsort(got["seq_col"].long() * T + got["seq_row"].long())
    ob = torch.argsort(want["seq_col"].long() * T + want["seq_row"].long())
    if not all(bool((got[k][oa] == want[k][ob]).all()) for k in got):
        raise RuntimeError(f"the call and the torch path disagree (T = {T})")
    for i in range(n_sets):
        call(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds, torch))
    return dict(T=T, N=N, K=K, Q=Q, L=L, sets=n_sets, bytes=one, us=us)


def report_seq(rows, torch, np):
    L = rows[0]["L"]
    out = ["phx_seq_batch against phx_train_batch(shuffle = 0) + a torch chop-pad-shuffle for the same sequences, and the bytes it needs",
           f"(tools/batch_time.py --seq {L}); B = 4 096, S = 9, D = 3 (SC64's shape, N = 36 864 columns), alternating keep (K = T N / 2), the",
           f"9-column PPO set in 16-word records, flags at 1 % of the elements per plane, max_seq_len = {L}, capacity = Q, advantages standardized,",
           "sequences shuffled, all six outputs written.  Expected bytes: 56 T N in, 72 Q L + 12 Q out.  One process, alternating, buffer sets",
           "rotated; median [min .. max] over the repeats, microseconds per call; TB/s = the expected bytes over the median.  The torch path is",
           "handed K and Q (no host wait).  Checked against that path before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"T = {r['T']:3d}  ({r['T'] * r['N'] / 1e6:.2f} M elements, K = {r['K'] / 1e6:.2f} M rows in Q = {r['Q'] / 1e6:.3f} M sequences = "
                   f"{r['Q'] * r['L'] / 1e6:.2f} M slots, {r['sets']} buffer sets of {r['bytes'] / 1e6:.1f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:62s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a = med["phx_seq_batch"]
        out.append(f"    the call: {r['bytes'] / 1e6:.2f} MB expected, {r['bytes'] / a / 1e6:.3f} TB/s = {r['bytes'] / (a * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak;  "
                   f"the torch path takes {med[SEQ_TORCH] / a:.2f}x")
    return "\n".join(out) + "\n"


def report(rows, torch, np):
    out = ["phx_train_batch against phx_traj_compact + torch for the same batch, and the bytes it needs (tools/batch_time.py); B = 4 096, S = 9,",
           "D = 3 (SC64's shape, N = 36 864 columns), alternating keep (K = T N / 2), the 9-column PPO set in 16-word records, advantages",
           "standardized, rows shuffled, out_row and out_col written.  Expected bytes: 52 T N in, 72 K out.  One process, alternating, buffer",
           "sets rotated; median [min .. max] over the repeats, microseconds per call; TB/s = the expected bytes over the median.  The torch",
           "path is handed K (no host wait).  Checked against that path before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"T = {r['T']:3d}  ({r['T'] * r['N'] / 1e6:.2f} M elements, K = {r['K'] / 1e6:.2f} M records, {r['sets']} buffer sets of {r['bytes'] / 1e6:.1f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:58s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a = med["phx_train_batch"]
        out.append(f"    the call: {r['bytes'] / 1e6:.2f} MB expected, {r['bytes'] / a / 1e6:.3f} TB/s = {r['bytes'] / (a * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak;  "
                   f"the torch path takes {med[TORCH] / a:.2f}x")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seq", type=int, default=None, metavar="L", help="time phx_seq_batch with max_seq_len = L instead (profiles/seq_time.txt)")
    ap.add_argument("--rows", type=int, nargs="+", default=list(TS), help="the T values (one of them alone: a kernel trace of that shape)")
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/batch_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    if args.seq is not None:
        for T in args.rows:
            rows.append(measure_seq(lib, _abi, torch, np, T, args.seq, args.seconds, args.repeats, dev))
            torch.cuda.empty_cache()
            print(report_seq(rows[-1:], torch, np).split("\n", 8)[-1], flush=True)
        with open(args.out or os.path.join(ROOT, "profiles", "seq_time.txt"), "w") as f:
            f.write(report_seq(rows, torch, np))
        sys.exit(0)
    for T in args.rows:
        rows.append(measure(lib, _abi, torch, np, T, args.seconds, args.repeats, dev))
        torch.cuda.empty_cache()
        print(report(rows[-1:], torch, np).split("\n", 7)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "batch_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
