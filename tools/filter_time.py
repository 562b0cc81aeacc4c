"""phx_filter_update and phx_filter_apply (include/phantom_amd_filter.h) against the same result in torch.
    python tools/filter_time.py [--out profiles/filter_time.txt] [--seconds 0.3] [--repeats 5] [--T 20 100]
GPU only: no device, no number.  Two shapes, both B = 4 096 env instances and D = 3 features: the plain chain's (S = 9 agents, every
element kept, one policy) and the 5-shop FSM chain's (S = 5, a keep plane with half the elements kept at random -- an FSM fragment's
holes -- and two policies, the agents alternating).  The planes are synthetic (stock-like values, 50 + 30 * N(0, 1)): the calls' work
depends on the shapes and the keep rate, not on the values.
What is timed.  update: one phx_filter_update call (five launches) into a running state.  apply: one phx_filter_apply call (one
launch), out of place, clip = 10.  The other path is torch on the same device tensors: update is, per policy, a masked mean and a
centred sum of squares in f64 and Chan's merge into device-resident count / mean / m2 tensors (no host wait); apply is a gather of
the per-column mean and denominator, (x - mean) / den, clamp and torch.where with the keep plane.
The tool first checks the calls against the torch path (means and M2 to 1e-9 relative, the normalised plane to 1e-5).  Then, in ONE
process, alternating, `repeats` windows of `seconds` each (HIP events around the window) after warm-up.  The share of HBM bandwidth of
apply counts the bytes the call must move -- the plane read and written and the keep bytes read -- over the 8 TB/s peak and the 6.3 TB/s
a streaming kernel reaches."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D = 4096, 3
SHAPES = (("plain chain", 9, False, 1), ("5-shop FSM chain", 5, True, 2))
CLIP = 10.0
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


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


def measure(lib, _abi, torch, name, S, holes, n_classes, T, seconds, repeats, dev):
    N = B * S
    gen = torch.Generator(device=dev).manual_seed(T + S)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    obs = 50.0 + 30.0 * torch.randn((T, N, D), generator=gen, dtype=torch.float32, device=dev)
    keep = (torch.rand((T, N), generator=gen, device=dev) < 0.5).to(torch.uint8) if holes else None
    cls = (torch.arange(N, device=dev) % S % n_classes).to(torch.int32) if n_classes > 1 else None
    state = torch.zeros((n_classes, _abi.FILTER_STATE_BYTES), dtype=torch.uint8, device=dev)
    ws = torch.empty(_abi.filter_workspace_bytes(N, D) // 8, dtype=torch.float64, device=dev)
    out = torch.empty_like(obs)
    p = lambda x: None if x is None else x.data_ptr()
    uio = _abi.PhxFilterUpdateIO(T=T, D=D, N=N, n_classes=n_classes, obs=p(obs), keep=p(keep), col_class=p(cls), state=p(state), workspace=p(ws))
    aio = _abi.PhxFilterApplyIO(T=T, D=D, N=N, n_classes=n_classes, clip=CLIP, obs=p(obs), keep=p(keep), col_class=p(cls), state=p(state), out=p(out))

    def call(fn, io):
        if getattr(lib, fn)(C.byref(io), stream) != 0:
            raise RuntimeError(lib.phx_last_error().decode())

    update = lambda i: call("phx_filter_update", uio)
    apply = lambda i: call("phx_filter_apply", aio)
    # the torch path: device-resident count / mean / m2 per policy
    t_count = torch.zeros(n_classes, dtype=torch.float64, device=dev)
    t_mean, t_m2 = torch.zeros((n_classes, D), dtype=torch.float64, device=dev), torch.zeros((n_classes, D), dtype=torch.float64, device=dev)
    kept = None if keep is None else keep != 0
    masks = [None if (kept is None and cls is None) else ((kept if kept is not None else True) & ((cls == c)[None, :] if cls is not None else True))
             for c in range(n_classes)]

    def update_torch(i):
        xd = obs.double()
        for c, m in enumerate(masks):
            if m is None:
                K = torch.tensor(float(T * N), dtype=torch.float64, device=dev)
                mb = xd.mean(dim=(0, 1))
                m2b = ((xd - mb) ** 2).sum(dim=(0, 1))
            else:
                w = m.unsqueeze(-1).double()
                K = w.sum()
                mb = (xd * w).sum(dim=(0, 1)) / K
                m2b = (((xd - mb) ** 2) * w).sum(dim=(0, 1))
            n = t_count[c] + K
            delta = mb - t_mean[c]
            t_m2[c] = t_m2[c] + m2b + delta * delta * (t_count[c] * K / n)
            t_mean[c] = t_mean[c] + delta * (K / n)
            t_count[c] = n

    def apply_torch(i):
        den = (t_m2 / (t_count - 1).unsqueeze(-1)).sqrt().float() + 1e-8
        mean = t_mean.float()
        if cls is not None:
            mean, den = mean[cls.long()], den[cls.long()]
        y = ((obs - mean) / den).clamp(-CLIP, CLIP)
        return y if kept is None else torch.where(kept.unsqueeze(-1), y, torch.zeros((), dtype=y.dtype, device=dev))

    update(0); update_torch(0); apply(0)
    want = apply_torch(0)
    torch.cuda.synchronize()
    st = state.cpu().numpy().reshape(-1).view(_abi.FILTER_STATE_DTYPE)
    import numpy as np
    if not (np.allclose(st["mean"][:, :D], t_mean.cpu().numpy(), rtol=1e-9) and np.allclose(st["m2"][:, :D], t_m2.cpu().numpy(), rtol=1e-9)
            and st["count"].tolist() == [int(v) for v in t_count.tolist()] and torch.allclose(out, want, rtol=1e-5, atol=1e-5)):
        raise RuntimeError(f"phx_filter_update / phx_filter_apply and the torch path disagree ({name}, T = {T})")
    nbytes = 2 * obs.numel() * 4 + (0 if keep is None else keep.numel())
    return [dict(what="update", shape=name, T=T, N=N, us=alternate(update, update_torch, seconds, repeats, torch), ours="phx_filter_update (5 launches)",
                 theirs="torch: masked f64 mean + centred M2 + Chan's merge", bytes=None),
            dict(what="apply", shape=name, T=T, N=N, us=alternate(apply, apply_torch, seconds, repeats, torch), ours="phx_filter_apply (1 launch)",
                 theirs="torch: (x - mean) / (std + 1e-8), clamp, where", bytes=nbytes)]


def report(rows, torch, np):
    out = ["phx_filter_update and phx_filter_apply against the same result in torch (tools/filter_time.py); B = 4 096, D = 3; the plain chain's",
           "shape (S = 9, all kept, one policy) and the 5-shop FSM chain's (S = 5, half the elements kept, two policies).  update: five launches",
           "into a running state, against a masked f64 mean, a centred sum of squares and Chan's merge per policy on device tensors.  apply: one",
           "launch, out of place, clip 10, against gather + (x - mean) / den + clamp + where.  One process, alternating; median [min .. max] over",
           "the repeats, microseconds per call.  Checked against the torch path before timing.",
           f"library: {os.path.basename(os.environ.get('PHX_LIB_PATH') or 'libphantom_amd.so (in-tree)')}",
           f"device: {torch.cuda.get_device_name()}", ""]
    for r in rows:
        med = {k: float(np.median(v)) for k, v in r["us"].items()}
        out.append(f"{r['what']:6s} {r['shape']:18s} T = {r['T']:3d}  N = {r['N']:6d}")
        for k, name in (("ours", r["ours"]), ("theirs", r["theirs"])):
            v = np.array(r["us"][k])
            out.append(f"    {name:58s} {med[k]:10.1f} us  [{v.min():.1f} .. {v.max():.1f}]  spread {(v.max() - v.min()) / max(med[k], 1e-9):.3f}")
        ratio = med["theirs"] / max(med["ours"], 1e-9)
        out.append(f"    the torch path takes {ratio:.2f}x" + ("" if ratio >= 1 else "   -- THE CALL IS SLOWER THAN TORCH HERE"))
        if r["bytes"]:
            rate = r["bytes"] / (med["ours"] * 1e-6)
            out.append(f"    {r['bytes'] / 1e6:.1f} MB moved: {rate / 1e12:.2f} TB/s, {rate / HBM_PEAK:.2f} of the 8 TB/s peak, {rate / HBM_STREAM:.2f} of the "
                       "6.3 TB/s a streaming kernel reaches")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--T", type=int, nargs="+", default=[20, 100], help="the fragment lengths")
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    from phantom_amd import _abi
    if not torch.cuda.is_available():
        sys.exit("tools/filter_time.py needs a GPU: a time measured anywhere else says nothing")
    lib = _abi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for name, S, holes, n_classes in SHAPES:
        for T in args.T:
            got = measure(lib, _abi, torch, name, S, holes, n_classes, T, args.seconds, args.repeats, dev)
            rows += got
            torch.cuda.empty_cache()
            print(report(got, torch, np).split("\n", 8)[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "filter_time.txt"), "w") as f:
        f.write(report(rows, torch, np))
