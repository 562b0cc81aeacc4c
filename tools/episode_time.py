"""phx_episode_stats (include/phantom_amd_episodes.h) against the same result in torch on the same device and against the bytes it needs.
    python tools/episode_time.py [--out profiles/episode_time.txt] [--seconds 0.5] [--repeats 5]
GPU only: no device, no number.  B = 4 096 env instances of SC64's trajectory shape (S = 9 agents, N = 9 B = 36 864 input columns),
T = 20 and 100 rows, 10-step episodes (every agent truncated in rows 9, 19, ..), the planes PhantomEnv.sample() passes on a plain
env -- reward, truncated, terminated; no acted, no reward_valid -- with the carry and the reduction, in four variants:
    G = 1, K = S   one output column per (env, agent), a class per agent: what EpisodeStats asks for the agent level
    G = S, K = 1   one output column per env instance, one class: the env level (a lane walks its S input columns)
each without and with the two per-row planes (episode_return, episode_len).
The tool first checks the call against torch: counts, lengths and the per-row lengths exactly, the returns to T 2^-23 times the sum
of the |rewards| of the episode's rows (torch sums an episode by a cumsum difference: another order).  Then, in ONE process,
alternating, `repeats` windows of `seconds` each (HIP events around the window), buffer sets rotated over more than 256 MB: the
call, and the same result in torch ops -- a cumulative sum over the rows, differences at the closing rows, sums / min / max per class.
Expected bytes per call (each plane read or written once): 6 T N in (reward 4, two flag planes 1 + 1), 8 T C for the per-row planes,
(48 + 2 * 8) C for col_stats and the carry in and out, 48 C read again by the reduction."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
B, S, EPISODE = 4096, 9, 10
TS = (20, 100)


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


def expected_bytes(T, N, G, planes):
    Cn = N // G
    return 6 * T * N + (8 * T * Cn if planes else 0) + (48 + 16) * Cn + 48 * Cn


def make_set(torch, T, N, G, K, planes, gen, dev):
    Cn = N // G
    rows = torch.arange(T, device=dev)
    p = dict(reward=torch.randn((T, N), generator=gen, device=dev), truncated=torch.zeros((T, N), dtype=torch.uint8, device=dev),
             terminated=torch.zeros((T, N), dtype=torch.uint8, device=dev))
    p["truncated"][(rows + 1) % EPISODE == 0] = 1
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    out = dict(carry_return=torch.zeros(Cn, device=dev), carry_len=torch.full((Cn,), -1, dtype=torch.int32, device=dev),
               episode_return=e((T, Cn), torch.float32) if planes else None, episode_len=e((T, Cn), torch.int32) if planes else None,
               col_stats=e((Cn, 48), torch.uint8), summary=e((K, 48), torch.uint8))
    return p, out


def in_torch(torch, p, G, K, planes):
    """the definition in torch ops for these planes (no masks, every member of a group flagged in the same rows, nothing open at
    the start): per class the count, the sum and the min / max of the episode returns and the length sum; the per-row planes"""
    r, tr, te = p["reward"], p["truncated"], p["terminated"]
    T, N = r.shape
    Cn = N // G
    rg = r.view(T, Cn, G).sum(dim=2) if G > 1 else r
    closes = ((tr != 0) | (te != 0)).view(T, Cn, G).all(dim=2)
    cs = rg.cumsum(0)
    rows = torch.arange(1, T + 1, device=r.device)[:, None].expand(T, Cn)
    close_row = torch.where(closes, rows, torch.zeros_like(rows))
    last_close = torch.cat([torch.zeros_like(rows[:1]), close_row[:-1]]).cummax(0).values      # the latest closing row before this one (1-based; 0: none)
    prev = torch.gather(torch.cat([torch.zeros((1, Cn), device=r.device), cs]), 0, last_close)      # the cumsum at the previous closing row
    ret = torch.where(closes, cs - prev, torch.zeros((), device=r.device))
    ln = torch.where(closes, rows - last_close, torch.full_like(rows, -1)).to(torch.int32)
    cl = closes.view(T, Cn // K, K)
    rk = ret.view(T, Cn // K, K).double()
    inf = torch.full((), float("inf"), dtype=torch.float64, device=r.device)
    res = dict(count=cl.sum(dim=(0, 1)), len_sum=torch.where(closes, ln, torch.zeros_like(ln)).view(T, Cn // K, K).sum(dim=(0, 1)),
               ret_sum=rk.sum(dim=(0, 1)), ret_min=torch.where(cl, rk, inf).amin(dim=(0, 1)), ret_max=torch.where(cl, rk, -inf).amax(dim=(0, 1)))
    if planes:
        res.update(episode_return=ret, episode_len=ln)
    return res


def measure(lib, _abi, torch, np, T, G, planes, seconds, repeats, dev):
    N, K = B * S, (S if G == 1 else 1)
    gen = torch.Generator(device=dev).manual_seed(0)
    one = expected_bytes(T, N, G, planes)
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets, ios = [], []
    ptr = lambda x: None if x is None else x.data_ptr()
    for _ in range(n_sets):
        p, out = make_set(torch, T, N, G, K, planes, gen, dev)
        sets.append((p, out))
        ios.append(_abi.PhxEpisodeIO(T=T, G=G, N=N, K=K, **{k: ptr(v) for k, v in p.items()}, **{k: ptr(v) for k, v in out.items()}))
    refs = [C.byref(io) for io in ios]

    def call(i):
        if lib.phx_episode_stats(refs[i % n_sets], stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    calls = {"phx_episode_stats": call, "torch: cumsum, differences at closing rows": lambda i: in_torch(torch, sets[i % n_sets][0], G, K, planes)}
    call(0)
    want = in_torch(torch, sets[0][0], G, K, True)
    torch.cuda.synchronize()
    p, out = sets[0]
    got = out["summary"].cpu().numpy().reshape(-1).view(_abi.EPISODE_STATS_DTYPE)
    size = float(p["reward"].abs().double().sum()) / (N // G)                     # the |rewards| of a column's rows, mean
    tol = T * 2.0 ** -23
    ok = (got["count"] == want["count"].cpu().numpy()).all() and (got["len_sum"] == want["len_sum"].cpu().numpy()).all()
    ok = ok and np.allclose(got["ret_sum"], want["ret_sum"].cpu().numpy(), rtol=0, atol=tol * size * (N // G // K))
    if planes:
        ok = ok and bool((out["episode_len"] == want["episode_len"]).all())
        ok = ok and bool(((out["episode_return"] - want["episode_return"]).abs() <= tol * p["reward"].abs().view(T, N // G, G).sum(dim=(0, 2))).all())
    if not ok:
        raise RuntimeError(f"kernel and torch disagree (T = {T}, G = {G}, planes = {planes})")
    episodes = int(got["count"].sum())
    del want
    for s in sets:                                        # (the check's call moved set 0's carry: every set starts as it was built)
        s[1]["carry_return"].zero_(); s[1]["carry_len"].fill_(-1)
    for i in range(n_sets):
        call(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds, torch))
    return dict(T=T, N=N, G=G, K=K, planes=planes, sets=n_sets, bytes=one, episodes=episodes, us=us)


def report(rows, torch, np):
    out = ["phx_episode_stats against the same result in torch and the bytes it needs (tools/episode_time.py); B = 4 096, S = 9 (SC64's shape,",
           "N = 36 864 input columns), 10-step episodes, reward + truncated + terminated given (6 B per element in), carry and reduction on.",
           "G = 1, K = 9: a column per (env, agent); G = 9, K = 1: a column per env.  Expected bytes: 6 T N in, 8 T C for the per-row planes,",
           "112 C for col_stats (written, read by the reduction) and the carry.  One process, alternating, buffer sets rotated; median",
           "[min .. max] over the repeats, microseconds per call; TB/s = the expected bytes over the median.  Checked against torch before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"T = {r['T']:3d}  G = {r['G']}  K = {r['K']}  per-row planes {'yes' if r['planes'] else 'no '}  ({r['T'] * r['N'] / 1e6:.2f} M elements, "
                   f"{r['episodes']} episodes closed per call, {r['sets']} buffer sets of {r['bytes'] / 1e6:.1f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            out.append(f"    {k:44s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / med[k]:.3f}")
        a = med["phx_episode_stats"]
        out.append(f"    the call: {r['bytes'] / 1e6:.2f} MB expected, {r['bytes'] / a / 1e6:.3f} TB/s = {r['bytes'] / (a * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak;  "
                   f"torch takes {med['torch: cumsum, differences at closing rows'] / a:.1f}x")
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
        sys.exit("tools/episode_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for T in TS:
        for G in (1, S):
            for planes in (False, True):
                rows.append(measure(lib, _abi, torch, np, T, G, planes, args.seconds, args.repeats, dev))
                torch.cuda.empty_cache()
                print(report(rows[-1:], torch, np).split("\n", 7)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "episode_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
