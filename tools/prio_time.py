"""phx_prio_add, phx_prio_update and phx_prio_sample (include/phantom_amd_prio.h) against the same result in torch.
    python tools/prio_time.py [--out profiles/prio_time.txt] [--seconds 0.3] [--repeats 5] [--log2-capacity 20 24] [--n 256 4096 65536]
GPU only: no device, no number.  The ring is tools/replay_time.py's: records of 32 words (128 bytes), K = 737 280 of them per add (SC64's
shape, B = 4 096, S = 9, T = 20), rings of C = 2^20 and 2^24 slots, minibatches of n = 256, 4 096 and 65 536.  The tree over 2^24 slots
is 76 MB (sum and min levels, 1.13 words per slot).
What is timed.  add: phx_prio_add alone, the count on the device (the ring's own add is not called in the window, so every call names the
same K slots: the work of a call does not depend on where they start).  update: phx_prio_update of the n slots of the last sample with
fresh priorities.  sample: phx_prio_sample + phx_replay_sample with slot_in, the records gathered.
The other path keeps the priorities as a flat f32 [C] tensor.  add: prios.index_fill_ of the K slots from a host cursor (K known on the
host: no wait charged).  update: prios.index_put_ + a running maximum.  sample: torch.multinomial(prios[:size], n, replacement=True) +
ring.index_select; multinomial takes at most 2^24 categories, so C = 2^24 is the largest ring it serves at all.
The tool first checks the calls: the root equals the leaves' sum to f32 accuracy, a sample's priorities are the leaves at its slots and
its records the ring's rows, and an update lands in the leaves.  Then, in ONE process, alternating, `repeats` windows of `seconds` each
(HIP events around the window) after warm-up."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, T = 4096, 9, 20
ROW_WORDS = 32
K = B * S * T
NS = (256, 4096, 65536)


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


def alternate(ours, theirs, seconds, repeats, torch):
    us = {"ours": [], "theirs": []}
    for _ in range(repeats):
        us["ours"].append(window(ours, seconds, torch))
        us["theirs"].append(window(theirs, seconds, torch))
    return us


def measure(lib, _abi, torch, log2c, ns, seconds, repeats, dev):
    Cn = 1 << log2c
    gen = torch.Generator(device=dev).manual_seed(log2c)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.randint(0, 2 ** 31 - 1, (K, ROW_WORDS), generator=gen, dtype=torch.int32, device=dev)
    count = torch.tensor([K], dtype=torch.int64, device=dev)
    ring, rstate = torch.zeros((Cn, ROW_WORDS), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    tree = torch.zeros(_abi.prio_layout(Cn)[3], dtype=torch.float32, device=dev)
    pstate = torch.zeros(32, dtype=torch.uint8, device=dev)
    flat, flat_max = torch.zeros(Cn, dtype=torch.float32, device=dev), torch.ones((), dtype=torch.float32, device=dev)
    host = dict(cursor=0)
    arange = torch.arange(K, device=dev)
    padd = _abi.PhxPrioAddIO(capacity=Cn, src_capacity=K, count_ptr=count.data_ptr(), ring_state=rstate.data_ptr(), tree=tree.data_ptr(),
                             state=pstate.data_ptr())
    radd = _abi.PhxReplayAddIO(capacity=Cn, src_capacity=K, row_words=ROW_WORDS, count_ptr=count.data_ptr(), src=src.data_ptr(), ring=ring.data_ptr(),
                               state=rstate.data_ptr())

    def call(fn, io):
        if getattr(lib, fn)(C.byref(io), stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    def add(i):
        call("phx_prio_add", padd)

    def ring_add():
        call("phx_replay_add", radd)

    def add_torch(i):
        first = max(0, K - Cn)
        flat.index_fill_(0, (host["cursor"] + arange[first:]) % Cn, 1.0)
        host["cursor"] = (host["cursor"] + K) % Cn

    for i in range(-(-Cn // K) + 1):                           # fill both until they have wrapped
        add(i); ring_add(); add_torch(i)
    torch.cuda.synchronize()
    L, off, W, words = _abi.prio_layout(Cn)
    root, leaves = float(tree[off[L]]), tree[:Cn]
    if rstate.tolist()[1] != Cn or not torch.equal(leaves, flat) or abs(root - float(leaves.double().sum())) > 1e-5 * root:
        raise RuntimeError(f"phx_prio_add and the torch path disagree (C = 2^{log2c}): root {root}, state {rstate.tolist()}")
    rows = [dict(what="add", C=Cn, n=K, us=alternate(add, add_torch, seconds, repeats, torch), ours="phx_prio_add",
                 theirs="torch: index_fill_ from a host cursor")]
    for n in ns:
        oslot, oprio = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        out = torch.empty((n, ROW_WORDS), dtype=torch.int32, device=dev)
        newp = torch.rand(n, generator=gen, device=dev) * 4 + 0.01
        sio = _abi.PhxPrioSampleIO(capacity=Cn, n=n, seed=1, draw=0, ring_state=rstate.data_ptr(), tree=tree.data_ptr(), out_slot=oslot.data_ptr(),
                                   out_priority=oprio.data_ptr())
        gio = _abi.PhxReplaySampleIO(capacity=Cn, n=n, row_words=ROW_WORDS, slot_in=oslot.data_ptr(), ring=ring.data_ptr(), state=rstate.data_ptr(),
                                     out=out.data_ptr())
        uio = _abi.PhxPrioUpdateIO(capacity=Cn, n=n, slot_in=oslot.data_ptr(), priority=newp.data_ptr(), ring_state=rstate.data_ptr(), tree=tree.data_ptr(),
                                   state=pstate.data_ptr())

        def sample(i):
            sio.draw = i                                      # a new stream of draws per call
            call("phx_prio_sample", sio)
            call("phx_replay_sample", gio)

        def sample_torch(i):
            return ring.index_select(0, torch.multinomial(flat, n, replacement=True))

        def update(i):
            call("phx_prio_update", uio)

        def update_torch(i):
            flat.index_put_((oslot,), newp)
            torch.maximum(flat_max, newp.max(), out=flat_max)

        sample(7)
        torch.cuda.synchronize()
        if not (torch.equal(out, ring[oslot]) and torch.equal(oprio, tree[oslot]) and int(oslot.min()) >= 0 and int(oslot.max()) < Cn):
            raise RuntimeError(f"phx_prio_sample's slots, priorities and records disagree (C = 2^{log2c}, n = {n})")
        update(0)
        torch.cuda.synchronize()
        want = torch.zeros(Cn, dtype=torch.float32, device=dev).index_reduce_(0, oslot, newp, "amax", include_self=True)
        if not torch.equal(tree[oslot], want[oslot]):
            raise RuntimeError(f"phx_prio_update's leaves are not the entries' maxima (C = 2^{log2c}, n = {n})")
        rows.append(dict(what="update", C=Cn, n=n, us=alternate(update, update_torch, seconds, repeats, torch), ours="phx_prio_update",
                         theirs="torch: index_put_ + running max"))
        rows.append(dict(what="sample", C=Cn, n=n, us=alternate(sample, sample_torch, seconds, repeats, torch), ours="phx_prio_sample + phx_replay_sample",
                         theirs="torch: multinomial + index_select"))
    return rows


def report(rows, torch, np):
    out = ["phx_prio_add, phx_prio_update and phx_prio_sample against the same result in torch (tools/prio_time.py); records of 128 bytes, K =",
           "737 280 per add (SC64's shape, B = 4 096, S = 9, T = 20).  add: the tree's call alone, the count on the device, against an index_fill_",
           "of a flat priority tensor from a host cursor.  update: n slots of a sample, against index_put_ + a running maximum.  sample: slots and",
           "priorities drawn and the records gathered, against torch.multinomial over the flat tensor + index_select.  One process, alternating;",
           "median [min .. max] over the repeats, microseconds per call.  Checked against the torch path before timing.",
           f"library: {os.path.basename(os.environ.get('PHX_LIB_PATH') or 'libphantom_amd.so (in-tree)')}",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"{r['what']:6s} C = 2^{r['C'].bit_length() - 1}  n = {r['n']:7d}")
        for k, name in (("ours", r["ours"]), ("theirs", r["theirs"])):
            v = np.array(r["us"][k])
            out.append(f"    {name:58s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / max(med[k], 1e-9):.3f}")
        ratio = med["theirs"] / max(med["ours"], 1e-9)
        out.append(f"    the torch path takes {ratio:.2f}x" + ("" if ratio >= 1 else "   -- THE CALL IS SLOWER THAN TORCH HERE"))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2-capacity", type=int, nargs="+", default=[20, 24], help="the ring sizes, as powers of two (at most 24: torch.multinomial)")
    ap.add_argument("--n", type=int, nargs="+", default=list(NS), help="the minibatch sizes")
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/prio_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for log2c in args.log2_capacity:
        got = measure(lib, _abi, torch, log2c, args.n, args.seconds, args.repeats, dev)
        rows += got
        torch.cuda.empty_cache()
        print(report(got, torch, np).split("\n", 8)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "prio_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
