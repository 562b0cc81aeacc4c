"""phx_gae (include/phantom_amd_gae.h) against the torch reverse loop a user would write without it, at SC64's trajectory planes.
    python tools/gae_time.py [--out profiles/gae_time.txt] [--seconds 0.5] [--repeats 5]
    python tools/gae_time.py --masked [--out profiles/gae_masked_time.txt]      phx_gae_masked against phx_gae, see below
GPU only: no device, no number.  Per shape the two are timed in ONE process, alternating, `repeats` times each over a window of
`seconds`, with HIP events; the kernel rotates over buffer sets whose total exceeds 256 MB, so that its planes come from HBM and not
from the Infinity Cache.  Roofline: the bytes the ALGORITHM needs, from the shapes -- 4 B per element of a value or output plane, 1 B
per element of a flag plane, a plane counted only when it is given, vf_next counted as the rows the definition reads -- over the
8 TB/s peak, as bench.py's `roofline` does.
--masked: phx_gae_masked_kernel at the same shapes, in the same process, alternating with phx_gae_kernel (the yardstick) under the same
rotation and windows, every plane given, with two acted planes: all one (reward_valid all one: the result is phx_gae's, checked bit for
bit) and alternating rows (an FSM supply chain: the shops act in even rows, their rewards arrive in odd rows and at an episode's end).
It moves 28 B per element against phx_gae's 22 (two more flag bytes, one more f32 output): 1.27 is the expected ratio.
    python tools/gae_time.py --vtrace [--out profiles/vtrace_time.txt]          phx_vtrace against phx_gae and the torch loop
--vtrace: phx_vtrace_kernel (include/phantom_amd_vtrace.h) with every plane given, at the same shapes, in the same process, alternating
with two yardsticks under the same rotation and windows: phx_gae_kernel, and the torch reverse loop of V-trace written here (the per-row
element-wise form of RLlib's from_importance_weights, with flags).  It first checks that the call with identical log-density planes
equals phx_gae's value_target bit for bit.  It moves 30 B per element against phx_gae's 22 (two more f32 inputs): 1.36 is the expected ratio.
    python tools/gae_time.py --traj [--out profiles/traj_next_time.txt]         phx_traj_next against phx_gae_masked and torch
--traj: phx_traj_next (include/phantom_amd_traj.h) at the same shapes with D = 3 and an FSM supply chain's planes (the shops act in even
rows and receive an observation from odd rows), every flag plane given, without and with next_obs, in the same process, alternating with
two yardsticks under the same rotation and windows: phx_gae_masked_kernel (unchanged), and the same result written in torch here (the
per-row reverse loop of selects, plus one torch.gather for next_obs).  It first checks the reduction case (no acted, no new_obs_valid:
next_row[t] == t, the step's own flags, next_obs == new_obs bit for bit) and that kernel and torch agree on every output.  Expectation: the
scan moves 10 B per element (four flag bytes in, six bytes out), the gather 5 + 8 D B per element that the result needs (acted, next_row,
one source word and one stored word per word; loading both candidate sources, as the kernel does, reads up to 4 D B more)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from phantom_amd import _abi

PEAK_BYTES_PER_S = 8e12
S, EPISODE = 9, 100                                       # SC64: 9 shops; 100-step episodes end in lock-step
SHAPES = ((4096, 100), (4096, 800), (65536, 100))         # (B, T)
GAMMA, LAMBDA = 0.99, 0.95


def algorithmic_bytes(T, N, cut_rows, vf_pred=True, vf_next=True, terminated=True, value_target=True):
    """bytes the definition reads and writes: reward + advantage, the planes that are given, vf_next at the rows it is read"""
    per_elem = 4 + 4 + 1 + (4 if vf_pred else 0) + (1 if terminated else 0) + (4 if value_target else 0)
    return T * N * per_elem + (4 * cut_rows * N if vf_next else 0)


def buffer_set(T, N, dev, gen):
    f = lambda: torch.randn((T, N), generator=gen, device=dev)
    trunc = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    trunc[EPISODE - 1::EPISODE] = 1
    return dict(reward=f(), vf_pred=f(), vf_next=f(), terminated=torch.zeros_like(trunc), truncated=trunc,
                advantage=torch.empty((T, N), device=dev), value_target=torch.empty((T, N), device=dev))


def gae_io(b, T, N):
    return _abi.PhxGaeIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, **{k: v.data_ptr() for k, v in b.items()})


def torch_loop(b, adv, vt):
    """the same quantities with element-wise torch ops, one row at a time (what the kernel replaces)"""
    r, v, vn = b["reward"], b["vf_pred"], b["vf_next"]
    term, cut = b["terminated"].bool(), (b["terminated"] | b["truncated"]).bool()
    T = r.shape[0]
    last = torch.zeros_like(r[0])
    zero = torch.zeros_like(r[0])
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            nv = torch.where(term[t], zero, vn[t])
            delta = r[t] + GAMMA * nv - v[t]
            last = delta
        else:
            nv = torch.where(term[t], zero, torch.where(cut[t], vn[t], v[t + 1]))
            delta = r[t] + GAMMA * nv - v[t]
            last = delta + (GAMMA * LAMBDA) * torch.where(cut[t], zero, last)
        adv[t] = last
    torch.add(adv, v, out=vt)


def window(fn, seconds):
    """microseconds per call of fn(i) over a window of about `seconds` (HIP events around the whole window)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(0); e1.record(); torch.cuda.synchronize()
    n = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for i in range(n):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, n


def measure(lib, B, T, seconds, repeats, dev):
    N = B * S
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * 22
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    sets = [buffer_set(T, N, dev, gen) for _ in range(n_sets)]
    ios = [gae_io(b, T, N) for b in sets]
    refs = [C.byref(io) for io in ios]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel(i):
        rc = lib.phx_gae(refs[i % n_sets], stream)
        if rc != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    adv_t, vt_t = torch.empty((T, N), device=dev), torch.empty((T, N), device=dev)
    loop = lambda i: torch_loop(sets[i % n_sets], adv_t, vt_t)
    kernel(0); loop(0); torch.cuda.synchronize()           # warm-up, and the two agree (f32, different association: a tolerance)
    err = float((sets[0]["advantage"] - adv_t).abs().max())
    if not err < 1e-3:
        raise RuntimeError(f"kernel and torch loop disagree: max |diff| = {err}")
    for i in range(n_sets):
        kernel(i)
    ks, ls = [], []
    for _ in range(repeats):                              # alternating
        ks.append(window(kernel, seconds)[0])
        ls.append(window(loop, seconds)[0])
    cut_rows = len(range(EPISODE - 1, T, EPISODE)) + (0 if T % EPISODE == 0 else 1)
    by = algorithmic_bytes(T, N, cut_rows)
    return dict(B=B, T=T, N=N, sets=n_sets, set_mb=one / 1e6, bytes=by, kernel_us=ks, loop_us=ls, max_abs_diff=err)


def measure_masked(lib, B, T, seconds, repeats, dev):
    N = B * S
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * 28
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets, plain, masked = [], [], {"all one": [], "alternating rows": []}
    for _ in range(n_sets):
        b = buffer_set(T, N, dev, gen)
        ones = torch.ones((T, N), dtype=torch.uint8, device=dev)
        alt, rv_alt = torch.zeros_like(ones), torch.zeros_like(ones)
        alt[0::2] = 1
        rv_alt[1::2] = 1; rv_alt[EPISODE - 1::EPISODE] = 1
        extra = dict(acted_one=ones, rv_one=ones.clone(), acted_alt=alt, rv_alt=rv_alt, reward_sum=torch.empty((T, N), device=dev),
                     adv_ref=torch.empty((T, N), device=dev), vt_ref=torch.empty((T, N), device=dev))
        sets.append((b, extra))
        plain.append(_abi.PhxGaeIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, **{**{k: v.data_ptr() for k, v in b.items()},
                                                                              "advantage": extra["adv_ref"].data_ptr(),
                                                                              "value_target": extra["vt_ref"].data_ptr()}))
        for name, a, rv in (("all one", "acted_one", "rv_one"), ("alternating rows", "acted_alt", "rv_alt")):
            masked[name].append(_abi.PhxGaeMaskedIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, acted=extra[a].data_ptr(), reward_valid=extra[rv].data_ptr(),
                                                    reward_sum=extra["reward_sum"].data_ptr(), **{k: v.data_ptr() for k, v in b.items()}))

    def caller(fn, ios):
        refs = [C.byref(io) for io in ios]

        def call(i):
            if fn(refs[i % n_sets], stream) != 0:
                raise RuntimeError(lib.phx_last_error().decode())
        return call

    calls = {"phx_gae_kernel": caller(lib.phx_gae, plain)}
    calls.update({f"phx_gae_masked_kernel, acted {k}": caller(lib.phx_gae_masked, v) for k, v in masked.items()})
    b, extra = sets[0]
    calls["phx_gae_kernel"](0); calls["phx_gae_masked_kernel, acted all one"](0); torch.cuda.synchronize()
    same = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in
               ((b["advantage"], extra["adv_ref"]), (b["value_target"], extra["vt_ref"]), (extra["reward_sum"], b["reward"])))
    if not same:
        raise RuntimeError("phx_gae_masked with all-one planes and phx_gae disagree")
    for fn in calls.values():
        for i in range(n_sets):
            fn(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds)[0])
    return dict(B=B, T=T, N=N, sets=n_sets, set_mb=one / 1e6, us=us)


CLIP = (1.0, 1.0, 1.0)                                    # RLlib's defaults: clip_rho_threshold, the trace clip, clip_pg_rho_threshold


def torch_vtrace_loop(b, vs, pg):
    """V-trace with element-wise torch ops, one row at a time: from_importance_weights' reverse loop, cut at the flags"""
    r, v, vn, bl, tl = b["reward"], b["vf_pred"], b["vf_next"], b["behaviour_logp"], b["target_logp"]
    term, cut = b["terminated"].bool(), (b["terminated"] | b["truncated"]).bool()
    T = r.shape[0]
    zero = torch.zeros_like(r[0])
    acc = zero
    for t in range(T - 1, -1, -1):
        rho = torch.exp(torch.clamp(tl[t] - bl[t], -20.0, 20.0))
        if t == T - 1:
            nv = nvs = torch.where(term[t], zero, vn[t])
            c = zero
        else:
            nv = torch.where(term[t], zero, torch.where(cut[t], vn[t], v[t + 1]))
            nvs = torch.where(term[t], zero, torch.where(cut[t], vn[t], vs[t + 1]))
            c = torch.where(cut[t], zero, acc)
        acc = torch.clamp(rho, max=CLIP[0]) * (r[t] + GAMMA * nv - v[t]) + (GAMMA * LAMBDA) * torch.clamp(rho, max=CLIP[1]) * c
        vs[t] = acc + v[t]
        pg[t] = torch.clamp(rho, max=CLIP[2]) * (r[t] + GAMMA * nvs - v[t])


def measure_vtrace(lib, B, T, seconds, repeats, dev):
    N = B * S
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * 30
    n_sets = max(2, -(-(256 << 20) // one) + 1)           # working set beyond the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sets, gae, vt = [], [], []
    for _ in range(n_sets):
        b = buffer_set(T, N, dev, gen)
        bl = torch.randn((T, N), generator=gen, device=dev) - 1.0
        b.update(behaviour_logp=bl, target_logp=bl + 0.7 * torch.randn((T, N), generator=gen, device=dev),
                 vs=torch.empty((T, N), device=dev), pg_advantage=torch.empty((T, N), device=dev))
        sets.append(b)
        gae.append(_abi.PhxGaeIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, **{k: b[k].data_ptr() for k in (
            "reward", "vf_pred", "vf_next", "terminated", "truncated", "advantage", "value_target")}))
        vt.append(_abi.PhxVtraceIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, rho_bar=CLIP[0], c_bar=CLIP[1], pg_rho_bar=CLIP[2], **{k: b[k].data_ptr() for k in (
            "reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp", "terminated", "truncated", "vs", "pg_advantage")}))

    def caller(fn, ios):
        refs = [C.byref(io) for io in ios]

        def call(i):
            if fn(refs[i % n_sets], stream) != 0:
                raise RuntimeError(lib.phx_last_error().decode())
        return call

    vs_t, pg_t = torch.empty((T, N), device=dev), torch.empty((T, N), device=dev)
    calls = {"phx_vtrace_kernel": caller(lib.phx_vtrace, vt), "phx_gae_kernel": caller(lib.phx_gae, gae),
             "torch loop": lambda i: torch_vtrace_loop(sets[i % n_sets], vs_t, pg_t)}
    b = sets[0]
    # identical log-density planes (the same pointer): vs is phx_gae's value_target, bit for bit
    same = _abi.PhxVtraceIO.from_buffer_copy(vt[0])
    same.target_logp = same.behaviour_logp
    if lib.phx_vtrace(C.byref(same), stream) != 0:
        raise RuntimeError(lib.phx_last_error().decode())
    calls["phx_gae_kernel"](0); torch.cuda.synchronize()
    if not bool((b["vs"].view(torch.int32) == b["value_target"].view(torch.int32)).all()):
        raise RuntimeError("phx_vtrace with identical log-density planes and phx_gae disagree")
    calls["phx_vtrace_kernel"](0); calls["torch loop"](0); torch.cuda.synchronize()       # and the kernel agrees with the loop (a tolerance)
    err = max(float((b["vs"] - vs_t).abs().max()), float((b["pg_advantage"] - pg_t).abs().max()))
    if not err < 1e-3:
        raise RuntimeError(f"kernel and torch loop disagree: max |diff| = {err}")
    for fn in (calls["phx_vtrace_kernel"], calls["phx_gae_kernel"]):
        for i in range(n_sets):
            fn(i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds)[0])
    return dict(B=B, T=T, N=N, sets=n_sets, set_mb=one / 1e6, us=us, max_abs_diff=err)


TRAJ_D = 3


def torch_traj_next(b, out, gather):
    """phx_traj_next with element-wise torch ops, one row at a time (the header's scan), and one torch.gather for next_obs"""
    tr, te, ac, nv = (b[k] != 0 for k in ("truncated", "terminated", "acted", "new_obs_valid"))
    T, N = tr.shape
    nr = torch.full((N,), -1, dtype=torch.int32, device=tr.device)
    term = torch.zeros((N,), dtype=torch.bool, device=tr.device)
    trunc = torch.zeros_like(term)
    minus, no = torch.full_like(nr, -1), torch.zeros_like(term)
    for t in range(T - 1, -1, -1):
        c = te[t] | tr[t] if t < T - 1 else torch.ones_like(term)
        here = torch.where(nv[t], torch.full_like(nr, t), minus)
        nr = torch.where(c, here, torch.where(nr < 0, here, nr))
        term = torch.where(c, te[t], term)
        trunc = torch.where(c, ~te[t] & tr[t], trunc)
        a = ac[t]
        out["next_row"][t] = torch.where(a, nr, minus)
        out["next_terminated"][t] = a & term
        out["next_truncated"][t] = a & trunc
        nr, term, trunc = torch.where(a, minus, nr), torch.where(a, no, term), torch.where(a, no, trunc)
    if gather:
        row = out["next_row"].to(torch.int64)
        src = b["new_obs"].gather(0, row.clamp(min=0)[..., None].expand(T, N, TRAJ_D))
        held = torch.where((row >= 0)[..., None], src, b["obs"])
        torch.where(ac[..., None], held, torch.zeros((), device=tr.device), out=out["next_obs"])


def measure_traj(lib, B, T, seconds, repeats, dev):
    N, D = B * S, TRAJ_D
    gen = torch.Generator(device=dev).manual_seed(0)
    one = T * N * (10 + 12 * D)
    n_sets = max(2, -(-(256 << 20) // (T * N * 10)) + 1)   # the scan's own planes alone exceed the 256 MiB Infinity Cache
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u8 = lambda: torch.zeros((T, N), dtype=torch.uint8, device=dev)
    sets, scan, both, masked = [], [], [], []
    for _ in range(n_sets):
        b = buffer_set(T, N, dev, gen)                   # (reward, value planes, flags, advantage, value_target: the yardstick's)
        acted, nvalid, rv = u8(), u8(), u8()
        acted[0::2] = 1
        nvalid[1::2] = 1; nvalid[EPISODE - 1::EPISODE] = 1
        rv[1::2] = 1; rv[EPISODE - 1::EPISODE] = 1
        b.update(acted=acted, new_obs_valid=nvalid, reward_valid=rv, reward_sum=torch.empty((T, N), device=dev),
                 obs=torch.randn((T, N, D), generator=gen, device=dev), new_obs=torch.randn((T, N, D), generator=gen, device=dev),
                 next_row=torch.empty((T, N), dtype=torch.int32, device=dev), next_terminated=u8(), next_truncated=u8(),
                 next_obs=torch.empty((T, N, D), device=dev))
        sets.append(b)
        p = lambda *ks: {k: b[k].data_ptr() for k in ks}
        flags = ("truncated", "terminated", "acted", "new_obs_valid", "next_row", "next_terminated", "next_truncated")
        scan.append(_abi.PhxTrajNextIO(T=T, D=D, N=N, **p(*flags)))
        both.append(_abi.PhxTrajNextIO(T=T, D=D, N=N, **p(*flags, "obs", "new_obs", "next_obs")))
        masked.append(_abi.PhxGaeMaskedIO(T=T, N=N, gamma=GAMMA, lambda_=LAMBDA, **p("reward", "vf_pred", "vf_next", "terminated", "truncated", "acted",
                                                                                      "reward_valid", "advantage", "value_target", "reward_sum")))

    def caller(fn, ios):
        refs = [C.byref(io) for io in ios]

        def call(i):
            if fn(refs[i % n_sets], stream) != 0:
                raise RuntimeError(lib.phx_last_error().decode())
        return call

    t_out = dict(next_row=torch.empty((T, N), dtype=torch.int32, device=dev), next_terminated=u8(), next_truncated=u8(),
                 next_obs=torch.empty((T, N, D), device=dev))
    calls = {"phx_traj_next, scan alone": caller(lib.phx_traj_next, scan), "phx_traj_next, scan + gather": caller(lib.phx_traj_next, both),
             "phx_gae_masked_kernel": caller(lib.phx_gae_masked, masked),
             "torch, scan alone": lambda i: torch_traj_next(sets[i % n_sets], t_out, False),
             "torch, scan + gather": lambda i: torch_traj_next(sets[i % n_sets], t_out, True)}
    b = sets[0]
    # the reduction case: no acted, no new_obs_valid
    red = _abi.PhxTrajNextIO.from_buffer_copy(both[0])
    red.acted = red.new_obs_valid = None
    if lib.phx_traj_next(C.byref(red), stream) != 0:
        raise RuntimeError(lib.phx_last_error().decode())
    torch.cuda.synchronize()
    te, tr = b["terminated"] != 0, b["truncated"] != 0
    ok = (bool((b["next_row"] == torch.arange(T, dtype=torch.int32, device=dev)[:, None]).all()) and bool(((b["next_terminated"] != 0) == te).all())
          and bool(((b["next_truncated"] != 0) == (~te & tr)).all())
          and bool((b["next_obs"].view(torch.int32) == b["new_obs"].view(torch.int32)).all()))
    if not ok:
        raise RuntimeError("phx_traj_next: the reduction case does not hold")
    calls["phx_traj_next, scan + gather"](0); calls["torch, scan + gather"](0); torch.cuda.synchronize()
    for k in ("next_row", "next_terminated", "next_truncated"):
        if not bool((b[k] == t_out[k]).all()):
            raise RuntimeError(f"kernel and torch disagree on {k}")
    if not bool((b["next_obs"].view(torch.int32) == t_out["next_obs"].view(torch.int32)).all()):
        raise RuntimeError("kernel and torch disagree on next_obs")
    for k in list(calls)[:3]:
        for i in range(n_sets):
            calls[k](i)
    us = {k: [] for k in calls}
    for _ in range(repeats):                              # alternating
        for k, fn in calls.items():
            us[k].append(window(fn, seconds)[0])
    return dict(B=B, T=T, N=N, sets=n_sets, set_mb=one / 1e6, us=us)


def report_traj(rows):
    D = TRAJ_D
    per = {"phx_traj_next, scan alone": 10, "phx_traj_next, scan + gather": 10 + 5 + 8 * D, "phx_gae_masked_kernel": 28,
           "torch, scan alone": 10, "torch, scan + gather": 10 + 5 + 8 * D}
    out = ["phx_traj_next against phx_gae_masked_kernel and the same result in torch (tools/gae_time.py --traj); SC64 planes, N = 9 B columns,",
           f"episodes of 100 steps, D = {D}, an FSM supply chain's acted / new_obs_valid planes (even rows / odd rows), every flag plane given.",
           f"Expected bytes per element: the scan 10 (four flag bytes in, six out), the gather 5 + 8 D = {5 + 8 * D}, phx_gae_masked 28.  One process,",
           "alternating, the same buffer rotation and windows.  Times: median [min .. max] over the repeats, microseconds per call; spread =",
           "(max - min) / median; TB/s = the expected bytes over the median.  The reduction case and kernel == torch on all four outputs are",
           "checked before timing.",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        el = r["T"] * r["N"]
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"B = {r['B']:6d}  T = {r['T']:4d}  ({el / 1e6:.1f} M elements, {r['sets']} buffer sets of {r['set_mb']:.0f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            m = med[k]
            line = (f"    {k:30s} {m:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / m:.3f}   {el * per[k] / m / 1e6:.2f} TB/s"
                    f" = {el * per[k] / (m * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak")
            if k == "phx_gae_masked_kernel":
                line += f"   scan alone takes {med['phx_traj_next, scan alone'] / m:.3f} of this (expected 10 / 28 = 0.357)"
            if k.startswith("torch"):
                line += f"   ratio to the kernel {m / med[k.replace('torch', 'phx_traj_next')]:.1f}x"
            out.append(line)
        g = med["phx_traj_next, scan + gather"] - med["phx_traj_next, scan alone"]
        out.append(f"    the gather by difference        {g:10.1f} us   {el * (5 + 8 * D) / g / 1e6:.2f} TB/s of its expected {5 + 8 * D} B per element")
    return "\n".join(out) + "\n"


def report_vtrace(rows):
    out = ["phx_vtrace_kernel against phx_gae_kernel and the torch reverse loop of V-trace (tools/gae_time.py --vtrace); SC64 planes, N = 9 B columns,",
           f"episodes of 100 steps, gamma = {GAMMA}, lambda = {LAMBDA}, thresholds {CLIP}, every plane given: 30 B per element moved against phx_gae's 22",
           "(expected ratio 1.36).  One process, alternating, the same buffer rotation and windows.  Times: median [min .. max] over the repeats,",
           "microseconds per call; spread = (max - min) / median.  With identical log-density planes vs equals phx_gae's value_target bit for bit",
           "(checked before timing).",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        el = r["T"] * r["N"]
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"B = {r['B']:6d}  T = {r['T']:4d}  ({el / 1e6:.1f} M elements, {r['sets']} buffer sets of {r['set_mb']:.0f} MB; max |kernel - loop| = "
                   f"{r['max_abs_diff']:.2e})")
        for k, v in r["us"].items():
            v = np.array(v)
            m = med[k]
            per = 22 if k == "phx_gae_kernel" else 30
            out.append(f"    {k:20s} {m:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / m:.3f}   {el * per / m / 1e6:.2f} TB/s"
                       f" = {el * per / (m * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak"
                       + ("" if k == "phx_vtrace_kernel" else f"   phx_vtrace_kernel takes {med['phx_vtrace_kernel'] / m:.4g} of this"))
    return "\n".join(out) + "\n"


def report_masked(rows):
    out = ["phx_gae_masked_kernel against phx_gae_kernel (tools/gae_time.py --masked); SC64 planes, N = 9 B columns, episodes of 100 steps,",
           f"gamma = {GAMMA}, lambda = {LAMBDA}, every plane given: 28 B per element moved against 22 (expected ratio 1.27).  One process, alternating,",
           "the same buffer rotation and windows.  Times: median [min .. max] over the repeats, microseconds per call; spread = (max - min) / median.",
           "With all-one planes the three outputs equal phx_gae's and the reward plane bit for bit (checked before timing).",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        el = r["T"] * r["N"]
        base = float(np.median(r["us"]["phx_gae_kernel"]))
        out.append(f"B = {r['B']:6d}  T = {r['T']:4d}  ({el / 1e6:.1f} M elements, {r['sets']} buffer sets of {r['set_mb']:.0f} MB)")
        for k, v in r["us"].items():
            v = np.array(v)
            m = float(np.median(v))
            per = 22 if k == "phx_gae_kernel" else 28
            out.append(f"    {k:44s} {m:9.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / m:.3f}   {el * per / m / 1e6:.2f} TB/s moved"
                       f" = {el * per / (m * 1e-6) / PEAK_BYTES_PER_S:.3f} of the peak   ratio to phx_gae_kernel {m / base:.3f}")
    return "\n".join(out) + "\n"


def report(rows):
    out = ["phx_gae_kernel against the torch reverse loop (tools/gae_time.py); SC64 planes, N = 9 B columns, episodes of 100 steps,",
           f"gamma = {GAMMA}, lambda = {LAMBDA}, every plane given.  Times: median [min .. max] over the repeats, microseconds per call.",
           f"device: {torch.cuda.get_device_name()}", ""]
    ok = True
    for r in rows:
        k, l = np.array(r["kernel_us"]), np.array(r["loop_us"])
        km, lm = float(np.median(k)), float(np.median(l))
        share = r["bytes"] / (km * 1e-6) / PEAK_BYTES_PER_S
        faster = bool(k.max() < l.min())
        ok &= faster
        out.append(f"B = {r['B']:6d}  T = {r['T']:4d}  ({r['bytes'] / 1e6:8.1f} MB algorithmic, {r['sets']} buffer sets of {r['set_mb']:.0f} MB)")
        out.append(f"    kernel      {km:10.1f} us  [{k.min():.1f} .. {k.max():.1f}]   {r['bytes'] / km / 1e6:.2f} TB/s = {share:.3f} of the 8 TB/s peak (memory-bound)")
        out.append(f"    torch loop  {lm:10.1f} us  [{l.min():.1f} .. {l.max():.1f}]   ratio {lm / km:.1f}x   kernel faster in every repeat: {'yes' if faster else 'NO'}"
                   f"   (max |kernel - loop| = {r['max_abs_diff']:.2e})")
    return "\n".join(out) + "\n", ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--masked", action="store_true", help="phx_gae_masked_kernel against phx_gae_kernel")
    ap.add_argument("--vtrace", action="store_true", help="phx_vtrace_kernel against phx_gae_kernel and the torch loop of V-trace")
    ap.add_argument("--traj", action="store_true", help="phx_traj_next against phx_gae_masked_kernel and the same result in torch")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/gae_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    if args.traj:
        for B, T in SHAPES:
            rows.append(measure_traj(lib, B, T, args.seconds, args.repeats, dev))
            torch.cuda.empty_cache()
            print(report_traj(rows[-1:]), flush=True)
        with open(args.out or os.path.join(ROOT, "profiles", "traj_next_time.txt"), "w") as f:
            f.write(report_traj(rows))
        sys.exit(0)
    if args.vtrace:
        for B, T in SHAPES:
            rows.append(measure_vtrace(lib, B, T, args.seconds, args.repeats, dev))
            torch.cuda.empty_cache()
            print(report_vtrace(rows[-1:]), flush=True)
        with open(args.out or os.path.join(ROOT, "profiles", "vtrace_time.txt"), "w") as f:
            f.write(report_vtrace(rows))
        sys.exit(0)
    if args.masked:
        for B, T in SHAPES:
            rows.append(measure_masked(lib, B, T, args.seconds, args.repeats, dev))
            torch.cuda.empty_cache()
            print(report_masked(rows[-1:]), flush=True)
        with open(args.out or os.path.join(ROOT, "profiles", "gae_masked_time.txt"), "w") as f:
            f.write(report_masked(rows))
        sys.exit(0)
    for B, T in SHAPES:
        rows.append(measure(lib, B, T, args.seconds, args.repeats, dev))
        torch.cuda.empty_cache()
        print(report(rows[-1:])[0], flush=True)
    text, ok = report(rows)
    with open(args.out or os.path.join(ROOT, "profiles", "gae_time.txt"), "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)
