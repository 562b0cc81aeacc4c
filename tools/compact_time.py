"""phx_traj_compact (include/phantom_amd_compact.h) against the same result in torch and against the bytes it needs, and what it
buys PhantomEnv.sample().
    python tools/compact_time.py [--out profiles/compact_time.txt] [--seconds 0.5] [--repeats 5]
GPU only: no device, no number.  SC64's three trajectory shapes (tools/gae_time.py: N = 9 B columns), the planes sample(compact=True)
hands to the call with a critic and D = 3 -- obs and new_obs (12 B), actions, rewards, trajectory_next_row, vf_preds, advantages,
value_targets (4 B), terminateds and truncateds (1 B): 50 B per element -- out_row given, keep in even rows (an FSM supply chain).  The
tool first checks every output against torch bit for bit.  Then, in ONE process, alternating, `repeats` windows of `seconds` each (HIP
events around the window), buffer sets rotated over more than 256 MB:
    the call;  the call without planes and index outputs (count + scan);  the same with T = 1 (the scan, and a count of one row);
    torch: movedim(0, 1) + boolean index per plane, on the device.
The count is the difference of the second and the third, the scatter the difference of the first and the second.  Expected bytes: in,
T N (1 + 50) once for the scatter and T N for the count; out, K (4 + 50) with out_row; plus 8 N for start each time it is written or read.
    python tools/compact_time.py --sample [--root TREE] [--modes plain,compact] [--out profiles/compact_sample_time.txt]
--sample: the number this exists for.  PhantomEnv.sample(T) + to_sample_batches() on the FSM supply chain of tests/test_gpu_compact.py
(5 shops, 8-step episodes) at B = 4 096, T = 20 and T = 100, wall clock with the copy to the host, 20 calls after 5 warm-up calls, per
mode: `plain` = sample(T), `compact` = sample(T, compact=True).  --root: import phantom_amd and tests/helpers.py from another tree (the
parent commit's, built there; `plain` only) -- one process per tree."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
S, D = 9, 3
SHAPES = ((4096, 100), (4096, 800), (65536, 100))         # (B, T)
PLANES = (("obs", 12), ("new_obs", 12), ("actions", 4), ("rewards", 4), ("terminateds", 1), ("truncateds", 1), ("trajectory_next_row", 4),
          ("vf_preds", 4), ("advantages", 4), ("value_targets", 4))
PLANE_BYTES = sum(eb for _, eb in PLANES)


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


def measure(lib, _abi, torch, B, T, seconds, repeats, dev):
    N = B * S
    cap = T * N
    K = ((T + 1) // 2) * N
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * (1 + PLANE_BYTES)
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets, full, offsets, scan = [], [], [], []
    for _ in range(n_sets):
        keep = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        keep[0::2] = 1
        src, dst = {}, {}
        for name, eb in PLANES:
            shape = (T, N) if eb <= 4 else (T, N, eb // 4)
            if eb == 1:
                src[name] = torch.randint(0, 2, shape, generator=gen, device=dev, dtype=torch.uint8)
            else:
                src[name] = torch.randn(shape, generator=gen, device=dev)
            dst[name] = torch.empty((K,) + shape[2:], dtype=src[name].dtype, device=dev)      # (K elements: what the call writes)
        b = dict(keep=keep, src=src, dst=dst, start=torch.empty(N + 1, dtype=torch.int64, device=dev),
                 out_row=torch.empty(K, dtype=torch.int32, device=dev))
        sets.append(b)
        io = _abi.PhxTrajCompactIO(T=T, n_planes=len(PLANES), N=N, capacity=K, keep=keep.data_ptr(), start=b["start"].data_ptr(),
                                   out_row=b["out_row"].data_ptr(), out_col=None)
        for k, (name, eb) in enumerate(PLANES):
            io.plane[k] = _abi.PhxCompactPlane(src=src[name].data_ptr(), dst=dst[name].data_ptr(), elem_bytes=eb, reserved=0)
        full.append(io)
        offsets.append(_abi.PhxTrajCompactIO(T=T, n_planes=0, N=N, capacity=K, keep=keep.data_ptr(), start=b["start"].data_ptr()))
        scan.append(_abi.PhxTrajCompactIO(T=1, n_planes=0, N=N, capacity=K, keep=keep.data_ptr(), start=b["start"].data_ptr()))

    def caller(ios):
        refs = [C.byref(io) for io in ios]

        def call(i):
            if lib.phx_traj_compact(refs[i % n_sets], stream) != 0:
                raise RuntimeError(lib.phx_last_error().decode())
        return call

    def in_torch(i):
        b = sets[i % n_sets]
        mask = b["keep"].movedim(0, 1) != 0
        return {name: x.movedim(0, 1)[mask] for name, x in b["src"].items()}

    calls = {"phx_traj_compact": caller(full), "count + scan (no planes)": caller(offsets), "scan (T = 1, no planes)": caller(scan),
             "torch: movedim + boolean index per plane": in_torch}
    b = sets[0]
    calls["phx_traj_compact"](0)
    want = in_torch(0)
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    if int(b["start"][N]) != K or not bool((b["start"][:N] == torch.arange(N, device=dev) * ((T + 1) // 2)).all()):
        raise RuntimeError("phx_traj_compact: start is wrong")
    if not bool((b["out_row"].view(N, -1) == torch.arange(0, T, 2, device=dev, dtype=torch.int32)).all()):
        raise RuntimeError("phx_traj_compact: out_row is wrong")
    for name, w in want.items():
        if tuple(w.shape) != tuple(b["dst"][name].shape) or not bool((bits(b["dst"][name]) == bits(w)).all()):
            raise RuntimeError(f"kernel and torch disagree on {name}")
    del want
    for k in list(calls)[:3]:
        for i in range(n_sets):
            calls[k](i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds, torch))
    return dict(B=B, T=T, N=N, K=K, sets=n_sets, set_mb=one / 1e6, us=us)


def report(rows, torch, np):
    out = ["phx_traj_compact against the same result in torch and the bytes it needs (tools/compact_time.py); SC64 planes, N = 9 B columns,",
           f"sample(compact=True)'s planes with a critic and D = {D}: {PLANE_BYTES} B per element in {len(PLANES)} planes, out_row given, keep in even rows.",
           "Expected bytes: the scatter T N (1 + 50) in and K (4 + 50) out plus 8 N of start; the count T N in and 8 N out; the scan 16 N.",
           "One process, alternating, buffer sets rotated; median [min .. max] over the repeats, microseconds per call; TB/s = the expected",
           "bytes over the median.  Every output is checked against torch bit for bit before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        T, N, K = r["T"], r["N"], r["K"]
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        by = {"scatter": T * N * (1 + PLANE_BYTES) + K * (4 + PLANE_BYTES) + 8 * N, "count": T * N + 8 * N, "scan": 16 * N}
        by["call"] = sum(by.values())
        out.append(f"B = {r['B']:6d}  T = {T:4d}  ({T * N / 1e6:.1f} M elements, K = {K / 1e6:.1f} M kept, {r['sets']} buffer sets of {r['set_mb']:.0f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:42s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a, b, c = med["phx_traj_compact"], med["count + scan (no planes)"], med["scan (T = 1, no planes)"]
        rate = lambda nbytes, us: f"{nbytes / us / 1e6:.2f} TB/s = {nbytes / (us * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak" if us > 0 else "n/a"
        out.append(f"    the call: {by['call'] / 1e6:.1f} MB expected, {rate(by['call'], a)};  torch takes {med['torch: movedim + boolean index per plane'] / a:.1f}x")
        out.append(f"    by difference: scatter {a - b:.1f} us ({rate(by['scatter'], a - b)}),  count {b - c:.1f} us ({rate(by['count'], b - c)}),  "
                   f"scan <= {c:.1f} us ({rate(by['scan'], c)})")
    return "\n".join(out) + "\n"


def sample_times(args, np):
    root = os.path.abspath(args.root) if args.root else ROOT
    sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
    import torch
    from helpers import supply_chain_env
    if not torch.cuda.is_available():
        sys.exit("tools/compact_time.py needs a GPU: a time measured anywhere else says nothing")
    out = [f"PhantomEnv.sample(T) + to_sample_batches() on the FSM supply chain (5 shops, 3 customers each, 8-step episodes), B = 4 096: wall clock",
           "with the copy to the host, milliseconds per call, 20 calls after 5 warm-up calls; median [min .. max]; rows = the batch's rows.",
           f"tree: {'the parent commit' if args.root else 'this one'};  device: {torch.cuda.get_device_name()}", ""]
    for T in (20, 100):
        for mode in args.modes.split(","):
            env = supply_chain_env(5, [3] * 5, 8, 4096, fsm=True, seed=5, exogenous="device")
            env.reset()
            kw = dict(compact=True) if mode == "compact" else {}
            ms, rows = [], 0
            for i in range(25):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cols = env.sample(T, **kw).to_sample_batches()["default_policy"]
                ms.append((time.perf_counter() - t0) * 1e3)
                rows = len(cols["obs"])
            v = np.array(ms[5:])
            out.append(f"T = {T:3d}  {mode:8s} {np.median(v):8.2f} ms  [{v.min():.2f} .. {v.max():.2f}]   rows {rows} of {T * 4096 * 5}")
            print(out[-1], flush=True)
            del env
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", action="store_true", help="wall clock of sample(T) + to_sample_batches(), plain and compact")
    ap.add_argument("--root", default=None, help="--sample: the tree to import phantom_amd and tests/helpers.py from")
    ap.add_argument("--modes", default="plain,compact")
    args = ap.parse_args()
    import numpy as np
    if args.sample:
        text = sample_times(args, np)
        with open(args.out or os.path.join(ROOT, "profiles", "compact_sample_time.txt"), "w") as f:
            f.write(text)
        sys.exit(0)
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/compact_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for B, T in SHAPES:
        rows.append(measure(lib, _abi, torch, B, T, args.seconds, args.repeats, dev))
        torch.cuda.empty_cache()
        print(report(rows[-1:], torch, np), flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "compact_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
