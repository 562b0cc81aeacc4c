"""phx_nstep (include/phantom_amd_nstep.h) against the same result in torch on the same device and against the bytes it needs.
    python tools/nstep_time.py [--out profiles/nstep_time.txt] [--seconds 0.5] [--repeats 5]
GPU only: no device, no number.  B = 4 096 env instances, T = 20 and 100 rows, n = 1, 3 and 10, D = 3, gamma = 0.99, two kinds of planes:
    plain  SC64's trajectory shape (N = 9 B columns): no acted, no next_row, every row a transition, 100-step episodes -- the fold and
           the gather;
    fsm    a 5-shop FSM supply chain (N = 5 B columns) with 8-step episodes: the shops act in even rows, a transition's observation
           arrives in the row after it (next_row = t + 1), the flag of the step that ends the episode stands at the episode's last
           trajectory row -- the successor scan, the fold and the gather.
The tool first checks the call against torch: the integer and flag planes and the gathered words bit for bit, the two float planes to
4 n 2^-24 sum_k |gamma^k r_k| (torch has no fmaf: its sum is addcmul, whose rounding is the compiler's choice; either side rounds p and
the sum at most n times each).  Then, in ONE process, alternating,
`repeats` windows of `seconds` each (HIP events around the window), buffer sets rotated over more than 256 MB: the call, and the same
result in torch -- the successor rows by a reversed cummin, then n rounds of gathers along the row axis with masks.
Expected bytes per element (each plane read or written once; what the hops read again is expected to hit in cache): plain 4 + 1 + 1 in,
18 out, the gather 4 + 12 in and 12 out: 52 B; fsm 4 + 1 + 1 + 1 + 4 in, succ_row 4 out and 4 in, 18 out, the gather 28: 65 B."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
B, D, GAMMA = 4096, 3, 0.99
KINDS = {"plain": dict(S=9, episode=100, bytes=52), "fsm": dict(S=5, episode=8, bytes=65)}
TS, NSTEPS = (20, 100), (1, 3, 10)


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


def planes(torch, kind, T, N, gen, dev):
    """one set of input planes [T, N] (next_obs [T, N, D]) of the kind, and its outputs"""
    ep = KINDS[kind]["episode"]
    rows = torch.arange(T, device=dev)
    p = dict(reward=torch.randn((T, N), generator=gen, device=dev), next_obs=torch.randn((T, N, D), generator=gen, device=dev),
             terminated=torch.zeros((T, N), dtype=torch.uint8, device=dev), truncated=torch.zeros((T, N), dtype=torch.uint8, device=dev))
    if kind == "plain":
        p["truncated"][(rows + 1) % ep == 0] = 1
        p["acted"] = p["next_row"] = None
    else:
        p["acted"] = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        p["acted"][0::2] = 1
        p["truncated"][(rows % ep) == ep - 2] = 1                # the episode's last trajectory row carries the flag of the step after it
        nr = torch.where(rows + 1 < T, rows + 1, torch.full_like(rows, -1)).to(torch.int32)
        p["next_row"] = torch.where(p["acted"] != 0, nr[:, None].expand(T, N), torch.full((T, N), -1, dtype=torch.int32, device=dev)).contiguous()
    e = lambda dtype, *tail: torch.empty((T, N) + tail, dtype=dtype, device=dev)
    out = dict(succ_row=e(torch.int32) if kind == "fsm" else None, nstep_reward=e(torch.float32), nstep_discount=e(torch.float32),
               nstep_last=e(torch.int32), nstep_terminated=e(torch.uint8), nstep_truncated=e(torch.uint8), nstep_next_row=e(torch.int32),
               nstep_next_obs=e(torch.float32, D))
    return p, out


def in_torch(torch, p, n, gamma):
    """the definition in torch ops: the successor rows, then n rounds of gathers along the row axis with masks"""
    r, tr, te, ac, nr, ob = (p[k] for k in ("reward", "truncated", "terminated", "acted", "next_row", "next_obs"))
    T, N = r.shape
    dev = r.device
    rows = torch.arange(T, device=dev)[:, None].expand(T, N)
    if ac is None:
        succ = torch.where(rows + 1 < T, rows + 1, torch.full_like(rows, -1))
        act = torch.ones((T, N), dtype=torch.bool, device=dev)
    else:
        act = ac != 0
        own = torch.where(act, rows, torch.full_like(rows, T))
        later = torch.cat([own[1:], torch.full((1, N), T, dtype=own.dtype, device=dev)])       # rows t + 1 ..
        succ = later.flip(0).cummin(0).values.flip(0)
        succ = torch.where(succ < T, succ, torch.full_like(succ, -1))
    term_p, trunc_p = te != 0, (te == 0) & (tr != 0)
    nr_p = rows if nr is None else nr.to(torch.int64)
    u, active = rows.clone(), act.clone()
    G, pw = torch.zeros_like(r), torch.ones_like(r)
    last, lnr = torch.full_like(rows, -1), torch.full_like(rows, -1)
    lte, ltr = torch.zeros_like(act), torch.zeros_like(act)
    for hop in range(n):
        term, trunc, nru, ru, su = term_p.gather(0, u), trunc_p.gather(0, u), nr_p.gather(0, u), r.gather(0, u), succ.gather(0, u)
        cmp = term | trunc | (nru >= 0)
        fold = active & cmp if hop else active
        G = torch.where(fold, ru if hop == 0 else torch.addcmul(G, pw, ru), G)
        pw = torch.where(fold, pw * gamma, pw)
        last, lnr = torch.where(fold, u, last), torch.where(fold, nru, lnr)
        lte, ltr = torch.where(fold, term, lte), torch.where(fold, trunc, ltr)
        active = fold & cmp & ~term & ~trunc & (su >= 0)
        u = torch.where(active, su, u)
    zero = torch.zeros((), dtype=r.dtype, device=dev)
    nob = ob.gather(0, last.clamp(min=0)[..., None].expand(T, N, ob.shape[-1]))
    return dict(nstep_reward=torch.where(act, G, zero), nstep_discount=torch.where(act, pw, zero), nstep_last=last.to(torch.int32),
                nstep_terminated=lte.to(torch.uint8), nstep_truncated=ltr.to(torch.uint8), nstep_next_row=lnr.to(torch.int32),
                nstep_next_obs=torch.where((last >= 0)[..., None], nob, zero))


def measure(lib, _abi, torch, kind, T, n, seconds, repeats, dev):
    N = B * KINDS[kind]["S"]
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * KINDS[kind]["bytes"]
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets, ios = [], []
    ptr = lambda x: None if x is None else x.data_ptr()
    for _ in range(n_sets):
        p, out = planes(torch, kind, T, N, gen, dev)
        sets.append((p, out))
        ios.append(_abi.PhxNstepIO(T=T, D=D, N=N, n=n, gamma=GAMMA, **{k: ptr(v) for k, v in p.items()}, **{k: ptr(v) for k, v in out.items()}))
    refs = [C.byref(io) for io in ios]

    def call(i):
        if lib.phx_nstep(refs[i % n_sets], stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    gamma32 = float(torch.tensor(GAMMA, dtype=torch.float32))
    calls = {"phx_nstep": call, "torch: n rounds of masked gathers": lambda i: in_torch(torch, sets[i % n_sets][0], n, gamma32)}
    call(0)
    want = in_torch(torch, sets[0][0], n, gamma32)
    torch.cuda.synchronize()
    got = sets[0][1]
    size = in_torch(torch, dict(sets[0][0], reward=sets[0][0]["reward"].abs()), n, gamma32)["nstep_reward"]      # sum_k |gamma^k r_k|
    for k, w in want.items():
        if k in ("nstep_reward", "nstep_discount"):               # (each side rounds p and the sum at most n times each: 2 n 2^-24 per side)
            ok = bool(((got[k] - w).abs() <= 4 * n * 2.0 ** -24 * (size if k == "nstep_reward" else w)).all())
        else:
            ok = bool((got[k].view(torch.int32) == w.view(torch.int32)).all()) if w.dtype == torch.float32 else bool((got[k] == w).all())
        if not ok:
            raise RuntimeError(f"kernel and torch disagree on {k} ({kind}, T = {T}, n = {n})")
    folded = float((torch.log(want["nstep_discount"][want["nstep_last"] >= 0]) / torch.log(torch.tensor(gamma32))).mean())
    del want
    for i in range(n_sets):
        call(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds, torch))
    return dict(kind=kind, T=T, N=N, n=n, sets=n_sets, set_mb=one / 1e6, bytes=one, folded=folded, us=us)


def report(rows, torch, np):
    out = ["phx_nstep against the same result in torch and the bytes it needs (tools/nstep_time.py); B = 4 096, D = 3, gamma = 0.99.",
           "plain: SC64's shape, N = 36 864 columns, no acted / next_row, 100-step episodes: 52 B per element expected (in 6, out 18, gather 28).",
           "fsm: 5 shops, N = 20 480 columns, acted in even rows, next_row = t + 1, 8-step episodes: 65 B per element expected (in 11, succ_row 4 + 4,",
           "out 18, gather 28).  One process, alternating, buffer sets rotated; median [min .. max] over the repeats, microseconds per call;",
           "TB/s = the expected bytes over the median; `folded` = transitions folded per trajectory row, mean.  Checked against torch before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"{r['kind']:5s} T = {r['T']:3d}  n = {r['n']:2d}  ({r['T'] * r['N'] / 1e6:.2f} M elements, folded {r['folded']:.2f}, {r['sets']} buffer sets of {r['set_mb']:.0f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:36s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a = med["phx_nstep"]
        out.append(f"    the call: {r['bytes'] / 1e6:.1f} MB expected, {r['bytes'] / a / 1e6:.2f} TB/s = {r['bytes'] / (a * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak;  "
                   f"torch takes {med['torch: n rounds of masked gathers'] / a:.1f}x")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/nstep_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for kind in KINDS:
        for T in TS:
            for n in NSTEPS:
                rows.append(measure(lib, _abi, torch, kind, T, n, args.seconds, args.repeats, dev))
                torch.cuda.empty_cache()
                print(report(rows[-1:], torch, np).split("\n", 7)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "nstep_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
