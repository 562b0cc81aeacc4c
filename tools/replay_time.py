"""phx_replay_add and phx_replay_sample (include/phantom_amd_replay.h) against the same result in torch, and against the bytes they move.
    python tools/replay_time.py [--out profiles/replay_time.txt] [--seconds 0.3] [--repeats 5] [--log2-capacity 20 24] [--n 256 4096 65536]
GPU only: no device, no number.  The records are those of SC64's shape (B = 4 096 env instances, S = 9 agents, D = 3) after T = 20
rows with the DQN column set that n_step = 3 produces -- obs, new_obs and nstep_new_obs (3 words each), actions, rewards, nstep_rewards,
nstep_discounts and four flag columns: 17 words in a 32-word record of 128 bytes -- K = 737 280 of them per add.  Rings of C = 2^20
records (128 MiB: inside the Infinity Cache) and 2^24 (2 GiB: far outside it); minibatches of n = 256, 4 096 and 65 536.
The other path.  Add: K read on the host, then ring.index_copy_(0, (cursor + arange(K)) % C, records[:K]), the cursor kept on the host.
Sample: torch.randint(size, (n,)) and ring.index_select(0, slots), size known on the host.
The tool first checks the calls against that path: the two rings hold the same bytes after adds that wrap, and a sample's records
are the ring's rows at its out_slot.  Then, in ONE process, alternating, `repeats` windows of `seconds` each (HIP events around the
window) after warm-up; the add rotates over source batches of more than 256 MB in all.  Bytes per add: 2 * 128 K (each record read
once and written once); per sample: (2 * 128 + 8) n."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
B, S, T = 4096, 9, 20
ROW_WORDS = 32
K = B * S * T
NS = (256, 4096, 65536)
N_SRC = 4                                                  # source batches the add rotates over: 4 * 94 MB
TORCH_ADD = "torch: K to the host, index_copy_"
TORCH_SAMPLE = "torch: randint + index_select"


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


def measure(lib, _abi, torch, log2c, ns, seconds, repeats, dev):
    Cn = 1 << log2c
    gen = torch.Generator(device=dev).manual_seed(log2c)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    srcs = [torch.randint(0, 2 ** 31 - 1, (K, ROW_WORDS), generator=gen, dtype=torch.int32, device=dev) for _ in range(N_SRC)]
    count = torch.tensor([K], dtype=torch.int64, device=dev)
    ring, state = torch.zeros((Cn, ROW_WORDS), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    other = torch.zeros_like(ring)
    host = dict(cursor=0, size=0)
    add_ios = [_abi.PhxReplayAddIO(capacity=Cn, src_capacity=K, row_words=ROW_WORDS, count_ptr=count.data_ptr(), src=s.data_ptr(),
                                   ring=ring.data_ptr(), state=state.data_ptr()) for s in srcs]
    add_refs = [C.byref(io) for io in add_ios]
    arange = torch.arange(K, device=dev)

    def add(i):
        if lib.phx_replay_add(add_refs[i % N_SRC], stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    def add_torch(i):
        k = int(count.item())                                # the wait a caller pays whose count lives on the device
        first = max(0, k - Cn)
        other.index_copy_(0, (host["cursor"] + arange[first:k]) % Cn, srcs[i % N_SRC][first:k])
        host["cursor"], host["size"] = (host["cursor"] + k) % Cn, min(Cn, host["size"] + k)

    fills = -(-Cn // K) + 1                                   # the check: the same adds into both rings until they have wrapped
    for i in range(fills):
        add(i)
        add_torch(i)
    torch.cuda.synchronize()
    st = state.tolist()
    if not torch.equal(ring, other) or st[:3] != [host["cursor"], Cn, fills * K] or st[3] != 0:
        raise RuntimeError(f"phx_replay_add and the torch path disagree (C = 2^{log2c}): state {st}")
    us = {"phx_replay_add": [], TORCH_ADD: []}
    for _ in range(repeats):                                  # alternating
        us["phx_replay_add"].append(window(add, seconds, torch))
        us[TORCH_ADD].append(window(add_torch, seconds, torch))
    rows = [dict(what="add", C=Cn, n=K, bytes=2 * 4 * ROW_WORDS * K, us=us, ours="phx_replay_add", theirs=TORCH_ADD)]
    for n in ns:
        out, oslot = torch.empty((n, ROW_WORDS), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        io = _abi.PhxReplaySampleIO(capacity=Cn, n=n, row_words=ROW_WORDS, seed=1, draw=0, ring=ring.data_ptr(), state=state.data_ptr(),
                                    out=out.data_ptr(), out_slot=oslot.data_ptr())
        ref = C.byref(io)

        def sample(i):
            io.draw = i                                       # a new stream of draws per call
            if lib.phx_replay_sample(ref, stream) != 0:
                raise RuntimeError(lib.phx_last_error().decode())

        def sample_torch(i):
            return ring.index_select(0, torch.randint(Cn, (n,), device=dev))

        sample(7)
        torch.cuda.synchronize()
        if not (torch.equal(out, ring[oslot]) and int(oslot.min()) >= 0 and int(oslot.max()) < Cn and (n < 4096 or oslot.unique().numel() > n // 2)):
            raise RuntimeError(f"phx_replay_sample's records are not the ring's rows at out_slot (C = 2^{log2c}, n = {n})")
        us = {"phx_replay_sample": [], TORCH_SAMPLE: []}
        for _ in range(repeats):
            us["phx_replay_sample"].append(window(sample, seconds, torch))
            us[TORCH_SAMPLE].append(window(sample_torch, seconds, torch))
        rows.append(dict(what="sample", C=Cn, n=n, bytes=(2 * 4 * ROW_WORDS + 8) * n, us=us, ours="phx_replay_sample", theirs=TORCH_SAMPLE))
    return rows


def report(rows, torch, np):
    out = ["phx_replay_add and phx_replay_sample against the same result in torch, and the bytes they move (tools/replay_time.py); records of",
           "SC64's shape (B = 4 096, S = 9, T = 20: K = 737 280 per add) with the DQN column set of n_step = 3, 17 words in a 32-word record of",
           "128 bytes.  Add: the count on the device (count_ptr), against K read on the host + index_copy_.  Sample: out and out_slot written,",
           "against torch.randint + index_select (size known on the host).  Bytes: 256 K per add, 264 n per sample.  One process, alternating;",
           "median [min .. max] over the repeats, microseconds per call; TB/s = the bytes over the median.  Checked against the torch path",
           "before timing.",
           f"library: {os.path.basename(os.environ.get('PHX_LIB_PATH') or 'libphantom_amd.so (in-tree)')}",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"{r['what']:6s} C = 2^{r['C'].bit_length() - 1} ({r['C'] * 4 * ROW_WORDS / 2 ** 20:.0f} MiB)  n = {r['n']:7d}  ({r['bytes'] / 1e6:.3f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:40s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a = med[r["ours"]]
        out.append(f"    the call: {r['bytes'] / a / 1e6:.3f} TB/s = {r['bytes'] / (a * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak;  the torch path takes "
                   f"{med[r['theirs']] / a:.2f}x")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2-capacity", type=int, nargs="+", default=[20, 24], help="the ring sizes, as powers of two")
    ap.add_argument("--n", type=int, nargs="+", default=list(NS), help="the minibatch sizes (one of them alone: a kernel trace of that shape)")
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/replay_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for log2c in args.log2_capacity:
        rows += measure(lib, _abi, torch, log2c, args.n, args.seconds, args.repeats, dev)
        torch.cuda.empty_cache()
        print(report(rows[-1 - len(args.n):], torch, np).split("\n", 9)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "replay_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
