"""FragmentOps on CPU tensors against a recording stand-in for the library: which pointer and which scalar lands in which field of
every io struct, and that every refusal comes before any call into the library.  No GPU, no built library: ``check_tensor`` and the
wrappers are pure host code, and ``_launch`` (the device guard and the stream) is the one seam that is stepped around."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from phantom_amd import _abi
from phantom_amd.fragment_ops import DeviceError, FragmentOps

T, B, S, D = 3, 2, 2, 3
SH, N = (T, B, S), B * S
ROW_WORDS, RING = 16, 8
f32, f64, u8, i32, i64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64


class RecordingLib:
    """every entry point records ``(name, a copy of the io struct)`` and returns ``rc``"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def phx_last_error(self):
        return b"stand-in"

    def __getattr__(self, entry):
        def call(io_ref, stream):
            io = io_ref._obj
            self.calls.append((entry, type(io).from_buffer_copy(io)))
            return self.rc
        return call


class Ops(FragmentOps):
    def _launch(self, entry, io):          # the seam: no torch.cuda.device guard, no stream
        self._check(getattr(self.lib, entry)(C.byref(io), None), entry)


def make_ops(rc=0):
    return Ops(RecordingLib(rc), torch.device("cpu"))


def z(dtype, *shape):
    return torch.zeros(shape or SH, dtype=dtype)


def p(x):
    return x.data_ptr()


def fields(io):
    """a struct as ``{field: value}``: a NULL pointer reads 0, an array is a list, a nested struct a dict"""
    out = {}
    for name, _ in io._fields_:
        v = getattr(io, name)
        if isinstance(v, C.Array):
            v = [fields(e) if isinstance(e, C.Structure) else e for e in v]
        out[name] = 0 if v is None else v
    return out


def misaligned(x):
    """``x``'s shape and dtype in a view that starts 4 bytes (8 for 8-byte elements) behind a 16-byte boundary"""
    nbytes, off = x.numel() * x.element_size(), max(4, x.element_size())
    raw = torch.zeros(nbytes + 16, dtype=u8)
    assert raw.data_ptr() % 16 == 0
    return raw[off:off + nbytes].view(x.dtype).view(x.shape)


def with_(kw, where, value):
    """``kw`` with one argument replaced; ``where``: a keyword, or (keyword, key or index) into a dict or tuple argument"""
    kw = dict(kw)
    if isinstance(where, tuple):
        key, k = where
        inner = kw[key]
        kw[key] = dict(inner, **{k: value}) if isinstance(inner, dict) else tuple(value if j == k else v for j, v in enumerate(inner))
    else:
        kw[where] = value
    return kw


def _cases():
    """per method: ``full`` (every optional argument given, all of `out` the caller's), ``bare`` (every optional one omitted) and
    ``planes``, the named tensors as (name in the message, where, is it the one that gives the leading shape)"""
    c = {}
    flags = dict(truncations=z(u8), terminations=z(u8))
    c["gae"] = SimpleNamespace(
        full=dict(rewards=z(f32), **flags, vf_pred=z(f32), vf_next=z(f32), gamma=0.5, lambda_=0.25, out=(z(f32), z(f32))),
        bare=dict(rewards=z(f32), truncations=z(u8)), lead="rewards",
        planes=["rewards", "truncations", "vf_pred", "vf_next", "terminations"])
    c["gae_masked"] = SimpleNamespace(
        full=dict(rewards=z(f32), **flags, vf_pred=z(f32), vf_next=z(f32), acted=z(u8), reward_valid=z(u8), gamma=0.5, lambda_=0.25,
                  out=(z(f32), z(f32), z(f32))),
        bare=dict(rewards=z(f32), truncations=z(u8)), lead="rewards",
        planes=["rewards", "truncations", "vf_pred", "vf_next", "terminations", "acted", "reward_valid"])
    c["vtrace"] = SimpleNamespace(
        full=dict(rewards=z(f32), **flags, vf_pred=z(f32), behaviour_logp=z(f32), target_logp=z(f32), vf_next=z(f32), gamma=0.5, lambda_=0.25,
                  clip_rho_threshold=2.0, clip_c_threshold=0.1, clip_pg_rho_threshold=0.5, out=(z(f32), z(f32))),
        bare=dict(rewards=z(f32), truncations=z(u8), vf_pred=z(f32), behaviour_logp=z(f32), target_logp=z(f32)), lead="rewards",
        planes=["rewards", "truncations", "vf_pred", "behaviour_logp", "target_logp", "vf_next", "terminations"])
    c["traj_next"] = SimpleNamespace(
        full=dict(**flags, acted=z(u8), new_obs_valid=z(u8), obs=z(f32, *SH, D), new_obs=z(f32, *SH, D),
                  out=(z(i32), z(u8), z(u8), z(f32, *SH, D))),
        bare=dict(truncations=z(u8)), lead="truncations",
        planes=["truncations", "terminations", "acted", "new_obs_valid", "obs", "new_obs"])
    c["nstep"] = SimpleNamespace(
        full=dict(rewards=z(f32), **flags, acted=z(u8), next_row=z(i32), next_obs=z(f32, *SH, D), n=3, gamma=0.5,
                  out=(z(f32), z(f32), z(i32), z(u8), z(u8), z(i32), z(f32, *SH, D), z(i32))),
        bare=dict(rewards=z(f32), truncations=z(u8)), lead="rewards",
        planes=["rewards", "truncations", "terminations", "acted", "next_row", "next_obs"])
    c["episode_stats"] = SimpleNamespace(
        full=dict(rewards=z(f32), **flags, acted=z(u8), reward_valid=z(u8), group=2, classes=2, carry=(z(f32, 2), z(i32, 2)), planes=True,
                  summary=True, out=(z(u8, 2, 48), z(u8, 2, 48), z(f32, T, 2), z(i32, T, 2))),
        bare=dict(rewards=z(f32), truncations=z(u8)), lead="rewards",
        planes=["rewards", "truncations", "terminations", "acted", "reward_valid", ("carry[0]", ("carry", 0)), ("carry[1]", ("carry", 1))])
    c["compact"] = SimpleNamespace(
        full=dict(keep=z(u8), planes={"a": z(f32), "b": z(i32, *SH, D), "c": z(u8)}, capacity=5,
                  out=(z(i64, N + 1), z(i32, 5), z(i32, 5), {"a": z(f32, 5), "b": z(i32, 5, D), "c": z(u8, 5)})),
        bare=dict(keep=z(u8), planes={}), lead="keep",
        planes=["keep", ("plane `a`", ("planes", "a")), ("plane `b`", ("planes", "b")), ("plane `c`", ("planes", "c"))])
    batch = dict(planes={"obs": z(f32, *SH, D), "rew": z(f32), "flag": z(u8)}, keep=z(u8), col_class=z(u8, S), class_id=1, standardize="rew",
                 shuffle=False, seed=7, epoch=9, row_words=ROW_WORDS, capacity=5, lead_dims=3)
    batch_planes = ["keep", "col_class", ("plane `obs`", ("planes", "obs")), ("plane `rew`", ("planes", "rew")), ("plane `flag`", ("planes", "flag"))]
    c["train_batch"] = SimpleNamespace(
        full=dict(batch, out=(z(i64, N + 1), z(i32, 5, ROW_WORDS), z(i32, 5), z(i32, 5), z(u8, 32), z(f64, N, 2))),
        bare=dict(planes={"rew": z(f32)}), lead="keep", planes=batch_planes)
    c["seq_batch"] = SimpleNamespace(
        full=dict(batch, max_seq_len=2, terminated=z(u8), truncated=z(u8),
                  out=(z(i64, N + 1), z(i32, 5, 2, ROW_WORDS), z(i32, 5), z(i32, 5), z(i32, 5), z(i32, 5, 2), z(i32, 5, 2), z(u8, 32),
                       z(f64, 3, N))),
        bare=dict(planes={"rew": z(f32)}, max_seq_len=2), lead="keep", planes=batch_planes + ["terminated", "truncated"])
    ring = dict(ring=z(i32, RING, ROW_WORDS), state=z(i64, 4))
    c["replay_add"] = SimpleNamespace(full=dict(ring, records=z(i32, 5, ROW_WORDS), count=z(i64, 1)), bare=dict(ring, records=z(i32, 5, ROW_WORDS)),
                                      lead=None, planes=["state", "count"])
    c["replay_sample"] = SimpleNamespace(full=dict(ring, n=5, seed=7, draw=9, slots=z(i64, 5), out=(z(i32, 5, ROW_WORDS), z(i64, 5))),
                                         bare=dict(ring, n=5), lead=None, planes=["state", "slots"])
    return c


CASES = _cases()


def _refusals():
    """``(method, match, kwargs)``: what the GPU files assert as refused, here for every named plane and every output"""
    r = []
    for op, case in CASES.items():
        full = case.full
        for plane in case.planes:
            name, where = plane if isinstance(plane, tuple) else (plane, plane)
            x = full[where[0]][where[1]] if isinstance(where, tuple) else full[where]
            bad = [x.to(torch.int16), x.to("meta")]                                    # dtype, device
            if x.numel() > 1:
                bad.append(x.new_zeros(tuple(x.shape) + (2,))[..., 0])                 # contiguity
            if where != case.lead:         # shape (a longer leading plane is a larger problem, refused for the next plane)
                bad.append(torch.cat([x, x[:1]]))
            r += [(op, re.escape(name), with_(full, where, v)) for v in bad]
        for i, x in enumerate(full.get("out", ())):
            if hasattr(x, "data_ptr"):
                r.append((op, rf"out\[{i}\]", with_(full, ("out", i), misaligned(x))))
                r.append((op, rf"out\[{i}\]", with_(full, ("out", i), x.to(torch.int16))))
    g = lambda op, match, **kw: r.append((op, match, dict(CASES[op].full, **kw)))
    for op in ("gae", "gae_masked", "vtrace"):
        g(op, "truncations", truncations=None)
        g(op, "gamma", gamma=1.5)
        g(op, "gamma", lambda_=-0.5)
        g(op, "`rewards` must be a", rewards=None)
        g(op, "`rewards` must be a", rewards=[[0.0]])              # a non-tensor: the op's own ValueError, as for None
        g(op, "T and N must be >= 1", rewards=z(f32, 0, B, S))
    g("gae_masked", "reward_valid", reward_valid=CASES["gae_masked"].full["reward_valid"][:, :-1].contiguous())
    g("vtrace", "vf_pred", vf_pred=None)
    g("vtrace", "target_logp", target_logp=z(f64))
    g("vtrace", "clip_c_threshold", clip_c_threshold=0.0)
    g("vtrace", "clip_rho_threshold", clip_rho_threshold=float("inf"))
    g("vtrace", "clip_rho_threshold", clip_pg_rho_threshold=1e-50)  # (0 as the f32 the struct holds)
    g("vtrace", r"out\[1\]", out=(z(f32), z(f32)[:-1]))
    g("traj_next", "come together", new_obs=None)                  # obs without new_obs
    g("traj_next", "come together", obs=None)                      # and the reverse
    g("traj_next", "`obs` must be a", obs=z(f32, *SH, 65), new_obs=z(f32, *SH, 65))
    g("traj_next", r"out\[3\]", obs=None, new_obs=None)            # a next_obs output without obs
    g("traj_next", "`out` is", out=CASES["traj_next"].full["out"][:3])
    for kw in (dict(n=0), dict(n=65), dict(n=2.0), dict(n=True), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan"))):
        g("nstep", "n =|gamma", **kw)
    g("nstep", "next_obs", next_obs=z(f64, *SH, D - 1))
    g("nstep", r"out\[6\]", next_obs=None)                         # a next_obs output without next_obs
    g("nstep", "`out` is", out=CASES["nstep"].full["out"][:6])
    for kw in (dict(group=0), dict(group=257), dict(group=True), dict(group=2.0), dict(classes=0), dict(classes=N + 1), dict(group=N + 1),
               dict(classes=True)):
        g("episode_stats", "group|classes", **kw)
    g("episode_stats", "carry", carry=(z(f32, 2), z(f32, 2)))
    g("episode_stats", "carry", carry=(z(f32, 2),))                # of the wrong length
    g("episode_stats", r"out\[0\]", group=1, carry=None)                       # col_stats sized for group = 2
    g("episode_stats", "`out` is", out=CASES["episode_stats"].full["out"][:3])
    full = CASES["compact"].full
    g("compact", "capacity", capacity=-1)
    g("compact", "out", out=full["out"][:3] + ({"a": full["out"][3]["a"]},))
    g("compact", r"out\[0\]", out=(full["out"][0][:-1],) + full["out"][1:])
    g("compact", "plane `b`", planes=dict(full["planes"], b=z(u8, *SH, D)))           # a trailing axis of u8
    g("compact", "plane `b`", planes=dict(full["planes"], b=z(f32, *SH, 65)))
    g("compact", r"out\[3\]\[`b`\]", out=full["out"][:3] + (dict(full["out"][3], b=misaligned(full["out"][3]["b"])),))
    for op, first in (("train_batch", 4), ("seq_batch", 7)):
        full = CASES[op].full
        for match, kw in (("standardize", dict(standardize="obs")), ("standardize", dict(standardize="nothing")), ("row_words", dict(row_words=6)),
                          ("row_words", dict(row_words=4)), ("row_words", dict(row_words=True)), ("capacity", dict(capacity=-1)),
                          (r"out\[1\]", dict(capacity=6)), ("class_id", dict(class_id=256)), ("class_id", dict(class_id=True)),
                          ("col_class", dict(col_class=z(u8, S + 1))), ("seed", dict(seed=-1)), ("epoch", dict(epoch=2 ** 64)),
                          ("`out` is", dict(out=full["out"][:-1])), (rf"out\[{first}\]", dict(out=full["out"][:-2] + (None, None))),
                          (rf"out\[{first}\].*need `standardize`", dict(standardize=None)),      # moments without standardize
                          ("lead_dims", dict(keep=None, lead_dims=5)), ("lead_dims", dict(keep=None, lead_dims=True)),
                          ("plane `rew`", dict(planes=dict(full["planes"], rew=z(f64)))),
                          ("planes", dict(planes={f"p{i}": z(f32) for i in range(33)}, standardize=None))):
            g(op, match, **kw)
    for bad in (0, 65537, 2.5, True, None):
        g("seq_batch", "max_seq_len", max_seq_len=bad)
    g("seq_batch", "capacity", capacity=5.0)                       # (train_batch and compact take int(capacity), seq_batch refuses it)
    g("seq_batch", "truncated", truncated=z(f32))
    g("seq_batch", "terminated", terminated=z(u8)[:2])
    ring, rec = CASES["replay_add"].full["ring"], CASES["replay_add"].full["records"]
    ring_bad = (ring.float(), ring.to("meta"), ring[:, :6], z(i32, RING, 6), ring[0], None, misaligned(ring))   # (6 words: no multiple of 4)
    for op in ("replay_add", "replay_sample"):
        for bad in ring_bad:
            g(op, "ring", ring=bad)
        g(op, "state", state=None)
    for match, kw in (("records", dict(records=rec[:, :4])), ("records", dict(records=rec.float())), ("records", dict(records=None)),
                      ("records", dict(records=misaligned(rec))), ("count", dict(count=6)), ("count", dict(count=-1)), ("count", dict(count=True)),
                      ("count", dict(count=2.0)), ("count", dict(count=z(i64, 2)))):
        g("replay_add", match, **kw)
    out = CASES["replay_sample"].full["out"]
    for match, kw in ((r"n = ", dict(n=0)), (r"n = ", dict(n=2.5)), (r"n = ", dict(n=True)), ("seed", dict(seed=-1)), ("draw", dict(draw=2 ** 64)),
                      ("slots", dict(slots=z(i64, 2))), (r"out\[0\]", dict(out=(out[0][:4], out[1]))), ("`out` is", dict(out=(out[0],)))):
        g("replay_sample", match, **kw)
    return r


REFUSALS = _refusals()


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[f"{op}-{k}" for k, (op, _, _) in enumerate(REFUSALS)])
def test_a_refusal_comes_before_any_call_into_the_library(k):
    op, match, kw = REFUSALS[k]
    ops = make_ops()
    with pytest.raises(ValueError, match=match):
        getattr(ops, op)(**kw)
    assert ops.lib.calls == []


def test_the_cases_and_the_refusals_cover_every_entry_point():
    assert set(CASES) == {e[len("phx_"):].replace("traj_compact", "compact") for e in _abi.FRAGMENT_OPS}
    assert {op for op, _, _ in REFUSALS} == set(CASES)


def test_nstep_tests_gamma_as_the_f32_the_struct_holds_and_the_gae_family_as_given():
    over = 1.0 + 1e-9                       # > 1 as given, 1 as an f32
    ops = make_ops()
    ops.nstep(**dict(CASES["nstep"].full, gamma=over))
    assert fields(ops.lib.calls[0][1])["gamma"] == 1.0
    for op in ("gae", "gae_masked", "vtrace"):
        ops = make_ops()
        with pytest.raises(ValueError, match="gamma"):
            getattr(ops, op)(**dict(CASES[op].full, gamma=over))
        assert ops.lib.calls == []


def test_a_failing_entry_point_raises_device_error_with_its_name_and_the_library_s_message():
    with pytest.raises(DeviceError, match=r"phx_gae failed \(7\): stand-in"):
        make_ops(rc=7).gae(**CASES["gae"].full)


def one_call(op, kw, entry):
    ops = make_ops()
    res = getattr(ops, op)(**kw)
    (name, io), = ops.lib.calls
    assert name == entry
    return res, fields(io)


def assert_allocated(res, want):
    """results allocated by the op: ``(dtype, shape)`` each (None: no tensor), 16-byte aligned"""
    assert len(res) == len(want)
    for x, w in zip(res, want):
        if w is None:
            assert x is None
        else:
            assert (x.dtype, tuple(x.shape)) == w and x.data_ptr() % 16 == 0 and x.is_contiguous() and x.device.type == "cpu"


def test_gae_marshalling():
    a = CASES["gae"].full
    res, io = one_call("gae", a, "phx_gae")
    assert io == dict(T=T, reserved0=0, N=N, gamma=0.5, lambda_=0.25, reward=p(a["rewards"]), vf_pred=p(a["vf_pred"]), vf_next=p(a["vf_next"]),
                      terminated=p(a["terminations"]), truncated=p(a["truncations"]), advantage=p(a["out"][0]), value_target=p(a["out"][1]))
    assert all(r is o for r, o in zip(res, a["out"]))
    b = CASES["gae"].bare
    res, io = one_call("gae", b, "phx_gae")
    assert_allocated(res, [(f32, SH)] * 2)
    assert io == dict(T=T, reserved0=0, N=N, gamma=float(np.float32(0.99)), lambda_=1.0, reward=p(b["rewards"]), vf_pred=0, vf_next=0, terminated=0,
                      truncated=p(b["truncations"]), advantage=p(res[0]), value_target=p(res[1]))


def test_gae_masked_marshalling():
    a = CASES["gae_masked"].full
    res, io = one_call("gae_masked", a, "phx_gae_masked")
    assert io == dict(T=T, reserved0=0, N=N, gamma=0.5, lambda_=0.25, reward=p(a["rewards"]), vf_pred=p(a["vf_pred"]), vf_next=p(a["vf_next"]),
                      terminated=p(a["terminations"]), truncated=p(a["truncations"]), acted=p(a["acted"]), reward_valid=p(a["reward_valid"]),
                      advantage=p(a["out"][0]), value_target=p(a["out"][1]), reward_sum=p(a["out"][2]))
    assert all(r is o for r, o in zip(res, a["out"]))
    b = CASES["gae_masked"].bare
    res, io = one_call("gae_masked", b, "phx_gae_masked")
    assert_allocated(res, [(f32, SH)] * 3)
    assert io == dict(T=T, reserved0=0, N=N, gamma=float(np.float32(0.99)), lambda_=1.0, reward=p(b["rewards"]), vf_pred=0, vf_next=0, terminated=0,
                      truncated=p(b["truncations"]), acted=0, reward_valid=0, advantage=p(res[0]), value_target=p(res[1]), reward_sum=p(res[2]))


def test_vtrace_marshalling_rounds_the_thresholds_to_f32():
    a = CASES["vtrace"].full
    res, io = one_call("vtrace", a, "phx_vtrace")
    assert io == dict(T=T, reserved0=0, N=N, gamma=0.5, lambda_=0.25, rho_bar=2.0, c_bar=float(np.float32(0.1)), pg_rho_bar=0.5, reserved1=0.0,
                      reward=p(a["rewards"]), vf_pred=p(a["vf_pred"]), vf_next=p(a["vf_next"]), behaviour_logp=p(a["behaviour_logp"]),
                      target_logp=p(a["target_logp"]), terminated=p(a["terminations"]), truncated=p(a["truncations"]), vs=p(a["out"][0]),
                      pg_advantage=p(a["out"][1]))
    assert all(r is o for r, o in zip(res, a["out"]))
    b = CASES["vtrace"].bare
    res, io = one_call("vtrace", b, "phx_vtrace")
    assert_allocated(res, [(f32, SH)] * 2)
    assert io == dict(T=T, reserved0=0, N=N, gamma=float(np.float32(0.99)), lambda_=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, reserved1=0.0,
                      reward=p(b["rewards"]), vf_pred=p(b["vf_pred"]), vf_next=0, behaviour_logp=p(b["behaviour_logp"]),
                      target_logp=p(b["target_logp"]), terminated=0, truncated=p(b["truncations"]), vs=p(res[0]), pg_advantage=p(res[1]))


def test_traj_next_marshalling():
    a = CASES["traj_next"].full
    res, io = one_call("traj_next", a, "phx_traj_next")
    assert io == dict(T=T, D=D, N=N, truncated=p(a["truncations"]), terminated=p(a["terminations"]), acted=p(a["acted"]),
                      new_obs_valid=p(a["new_obs_valid"]), obs=p(a["obs"]), new_obs=p(a["new_obs"]), next_row=p(a["out"][0]),
                      next_terminated=p(a["out"][1]), next_truncated=p(a["out"][2]), next_obs=p(a["out"][3]))
    assert all(r is o for r, o in zip(res, a["out"]))
    b = CASES["traj_next"].bare
    res, io = one_call("traj_next", b, "phx_traj_next")
    assert_allocated(res, [(i32, SH), (u8, SH), (u8, SH), None])
    assert io == dict(T=T, D=0, N=N, truncated=p(b["truncations"]), terminated=0, acted=0, new_obs_valid=0, obs=0, new_obs=0, next_row=p(res[0]),
                      next_terminated=p(res[1]), next_truncated=p(res[2]), next_obs=0)
    res, io = one_call("traj_next", dict(a, out=None), "phx_traj_next")                # with the gather: the fourth is allocated too
    assert_allocated(res, [(i32, SH), (u8, SH), (u8, SH), (f32, SH + (D,))])
    assert io["next_obs"] == p(res[3])


def test_nstep_marshalling_and_its_seven_or_eight_outputs():
    a = CASES["nstep"].full
    out = a["out"]
    res, io = one_call("nstep", a, "phx_nstep")
    want = dict(T=T, D=D, N=N, n=3, gamma=0.5, reward=p(a["rewards"]), truncated=p(a["truncations"]), terminated=p(a["terminations"]),
                acted=p(a["acted"]), next_row=p(a["next_row"]), next_obs=p(a["next_obs"]), succ_row=p(out[7]), nstep_reward=p(out[0]),
                nstep_discount=p(out[1]), nstep_last=p(out[2]), nstep_terminated=p(out[3]), nstep_truncated=p(out[4]), nstep_next_row=p(out[5]),
                nstep_next_obs=p(out[6]))
    assert io == want
    assert len(res) == 7 and all(r is o for r, o in zip(res, out))                    # the first seven are returned
    res, io = one_call("nstep", dict(a, out=out[:7]), "phx_nstep")                     # no eighth, with `acted`: succ_row is allocated here
    assert io["succ_row"] not in (0, p(out[7])) and io["succ_row"] % 16 == 0 and dict(io, succ_row=p(out[7])) == want
    res, io = one_call("nstep", dict(a, out=out[:7], acted=None), "phx_nstep")         # ... and not without `acted`
    assert io["succ_row"] == 0 and io["acted"] == 0
    b = CASES["nstep"].bare
    res, io = one_call("nstep", b, "phx_nstep")
    assert_allocated(res, [(f32, SH), (f32, SH), (i32, SH), (u8, SH), (u8, SH), (i32, SH), None])
    assert io == dict(T=T, D=0, N=N, n=3, gamma=float(np.float32(0.99)), reward=p(b["rewards"]), truncated=p(b["truncations"]), terminated=0,
                      acted=0, next_row=0, next_obs=0, succ_row=0, nstep_reward=p(res[0]), nstep_discount=p(res[1]), nstep_last=p(res[2]),
                      nstep_terminated=p(res[3]), nstep_truncated=p(res[4]), nstep_next_row=p(res[5]), nstep_next_obs=0)
    res, io = one_call("nstep", dict(a, out=None), "phx_nstep")                        # with the gather: the seventh is allocated too
    assert_allocated(res, [(f32, SH), (f32, SH), (i32, SH), (u8, SH), (u8, SH), (i32, SH), (f32, SH + (D,))])
    assert io["nstep_next_obs"] == p(res[6]) and io["succ_row"] not in (0, io["nstep_next_row"])


def test_episode_stats_marshalling_and_the_results_that_are_not_wanted():
    a = CASES["episode_stats"].full
    out = a["out"]
    res, io = one_call("episode_stats", a, "phx_episode_stats")
    want = dict(T=T, G=2, N=N, K=2, reserved0=0, reward=p(a["rewards"]), truncated=p(a["truncations"]), terminated=p(a["terminations"]),
                acted=p(a["acted"]), reward_valid=p(a["reward_valid"]), carry_return=p(a["carry"][0]), carry_len=p(a["carry"][1]),
                episode_return=p(out[2]), episode_len=p(out[3]), col_stats=p(out[0]), summary=p(out[1]))
    assert io == want and all(r is o for r, o in zip(res, out))
    res, io = one_call("episode_stats", dict(a, out=(out[0], None, None, None)), "phx_episode_stats")      # None where not wanted
    assert io == dict(want, episode_return=0, episode_len=0, summary=0) and res[0] is out[0] and res[1:] == (None, None, None)
    b = CASES["episode_stats"].bare
    res, io = one_call("episode_stats", b, "phx_episode_stats")
    assert_allocated(res, [(u8, (N, 48)), (u8, (1, 48)), None, None])
    assert io == dict(T=T, G=1, N=N, K=1, reserved0=0, reward=p(b["rewards"]), truncated=p(b["truncations"]), terminated=0, acted=0, reward_valid=0,
                      carry_return=0, carry_len=0, episode_return=0, episode_len=0, col_stats=p(res[0]), summary=p(res[1]))
    res, io = one_call("episode_stats", dict(b, planes=True, summary=False, classes=2), "phx_episode_stats")
    assert_allocated(res, [(u8, (N, 48)), None, (f32, (T, N)), (i32, (T, N))])
    assert (io["summary"], io["episode_return"], io["episode_len"], io["K"]) == (0, p(res[2]), p(res[3]), 2)


NO_PLANE = dict(src=0, dst=0, elem_bytes=0, reserved=0)


def test_compact_marshalling_one_launch_per_16_planes():
    a = CASES["compact"].full
    src, out = a["planes"], a["out"]
    res, io = one_call("compact", a, "phx_traj_compact")
    assert io == dict(T=T, n_planes=3, N=N, capacity=5, keep=p(a["keep"]), start=p(out[0]), out_row=p(out[1]), out_col=p(out[2]),
                      plane=[dict(src=p(src["a"]), dst=p(out[3]["a"]), elem_bytes=4, reserved=0),
                             dict(src=p(src["b"]), dst=p(out[3]["b"]), elem_bytes=4 * D, reserved=0),
                             dict(src=p(src["c"]), dst=p(out[3]["c"]), elem_bytes=1, reserved=0)] + [NO_PLANE] * 13)
    assert all(r is o for r, o in zip(res, out))
    res, io = one_call("compact", dict(a, out=(out[0], None, None, out[3])), "phx_traj_compact")          # out_row / out_col not wanted
    assert (io["out_row"], io["out_col"]) == (0, 0) and res[1] is None and res[2] is None
    b = CASES["compact"].bare                                                         # no plane at all: still one launch
    res, io = one_call("compact", b, "phx_traj_compact")
    assert_allocated(res[:3], [(i64, (N + 1,)), (i32, (T * N,)), (i32, (T * N,))])
    assert res[3] == {}
    assert io == dict(T=T, n_planes=0, N=N, capacity=T * N, keep=p(b["keep"]), start=p(res[0]), out_row=p(res[1]), out_col=p(res[2]),
                      plane=[NO_PLANE] * 16)
    res, _ = one_call("compact", dict(a, out=None, capacity=None), "phx_traj_compact")
    assert_allocated([res[3][k] for k in "abc"], [(f32, (T * N,)), (i32, (T * N, D)), (u8, (T * N,))])
    # 17 planes: two launches, the row / col pointers in the first only
    src = {f"p{i:02d}": z(f32) for i in range(17)}
    out = (z(i64, N + 1), z(i32, 5), z(i32, 5), {k: z(f32, 5) for k in src})
    ops = make_ops()
    ops.compact(a["keep"], src, 5, out=out)
    assert [name for name, _ in ops.lib.calls] == ["phx_traj_compact"] * 2
    first, second = (fields(io) for _, io in ops.lib.calls)
    head = dict(T=T, N=N, capacity=5, keep=p(a["keep"]), start=p(out[0]))
    plane = lambda k: dict(src=p(src[k]), dst=p(out[3][k]), elem_bytes=4, reserved=0)
    assert first == dict(head, n_planes=16, out_row=p(out[1]), out_col=p(out[2]), plane=[plane(k) for k in list(src)[:16]])
    assert second == dict(head, n_planes=1, out_row=0, out_col=0, plane=[plane("p16")] + [NO_PLANE] * 15)


def batch_planes(io, planes, layout):
    """plane[k] holds plane k's pointer, with word_off and elem_bytes as the returned layout says; the rest is zero"""
    want = [dict(src=p(x), elem_bytes=x.element_size() * layout[k][1], word_off=layout[k][0]) for k, x in planes.items()]
    return io["plane"] == want + [dict(src=0, elem_bytes=0, word_off=0)] * (_abi.BATCH_MAX_PLANES - len(want))


def test_train_batch_marshalling():
    a = CASES["train_batch"].full
    out = a["out"]
    res, io = one_call("train_batch", a, "phx_train_batch")
    layout = res[5]
    assert layout == {"obs": (0, D, f32), "rew": (D, 1, f32), "flag": (D + 1, 1, u8)}
    assert batch_planes(io, a["planes"], layout) and [e["elem_bytes"] for e in io["plane"][:3]] == [4 * D, 4, 1]
    del io["plane"]
    assert io == dict(T=T, N=N, capacity=5, n_planes=3, row_words=ROW_WORDS, S=S, class_id=1, std_plane=1, shuffle=0, seed=7, epoch=9,
                      keep=p(a["keep"]), col_class=p(a["col_class"]), start=p(out[0]), records=p(out[1]), out_row=p(out[2]), out_col=p(out[3]),
                      moments=p(out[4]), workspace=p(out[5]), reserved=[0, 0])
    assert all(r is o for r, o in zip(res[:5], out))
    b = CASES["train_batch"].bare
    res, io = one_call("train_batch", b, "phx_train_batch")
    assert_allocated(res[:5], [(i64, (N + 1,)), (i32, (T * N, 16)), (i32, (T * N,)), (i32, (T * N,)), None])
    assert res[5] == {"rew": (0, 1, f32)} and batch_planes(io, b["planes"], res[5])
    del io["plane"]
    assert io == dict(T=T, N=N, capacity=T * N, n_planes=1, row_words=16, S=1, class_id=0, std_plane=-1, shuffle=1, seed=0, epoch=0, keep=0,
                      col_class=0, start=p(res[0]), records=p(res[1]), out_row=p(res[2]), out_col=p(res[3]), moments=0, workspace=0, reserved=[0, 0])
    res, io = one_call("train_batch", dict(a, out=None, capacity=2.0), "phx_train_batch")          # int(capacity); moments and workspace
    assert_allocated(res[:5], [(i64, (N + 1,)), (i32, (2, ROW_WORDS)), (i32, (2,)), (i32, (2,)), (u8, (32,))])
    assert io["capacity"] == 2 and io["moments"] == p(res[4]) and io["workspace"] % 16 == 0 and io["workspace"] != 0


def test_seq_batch_marshalling_and_its_default_capacity():
    a = CASES["seq_batch"].full
    out = a["out"]
    res, io = one_call("seq_batch", a, "phx_seq_batch")
    layout = res[8]
    assert layout == {"obs": (0, D, f32), "rew": (D, 1, f32), "flag": (D + 1, 1, u8)}
    assert batch_planes(io, a["planes"], layout) and [e["elem_bytes"] for e in io["plane"][:3]] == [4 * D, 4, 1]
    del io["plane"]
    assert io == dict(T=T, N=N, capacity=5, n_planes=3, row_words=ROW_WORDS, S=S, class_id=1, std_plane=1, shuffle=0, seed=7, epoch=9,
                      keep=p(a["keep"]), col_class=p(a["col_class"]), seq_start=p(out[0]), records=p(out[1]), out_row=p(out[5]),
                      out_col=p(out[6]), moments=p(out[7]), workspace=p(out[8]), max_seq_len=2, terminated=p(a["terminated"]),
                      truncated=p(a["truncated"]), seq_lens=p(out[2]), seq_row=p(out[3]), seq_col=p(out[4]), reserved=[0, 0])
    assert all(r is o for r, o in zip(res[:8], out))
    b = CASES["seq_batch"].bare
    res, io = one_call("seq_batch", b, "phx_seq_batch")
    Q = N * 2                                                                           # N * ceil(T / L) without a flag plane
    assert_allocated(res[:8], [(i64, (N + 1,)), (i32, (Q, 2, 16)), (i32, (Q,)), (i32, (Q,)), (i32, (Q,)), (i32, (Q, 2)), (i32, (Q, 2)), None])
    assert res[8] == {"rew": (0, 1, f32)} and batch_planes(io, b["planes"], res[8])
    del io["plane"]
    assert io == dict(T=T, N=N, capacity=Q, n_planes=1, row_words=16, S=1, class_id=0, std_plane=-1, shuffle=1, seed=0, epoch=0, keep=0,
                      col_class=0, seq_start=p(res[0]), records=p(res[1]), out_row=p(res[5]), out_col=p(res[6]), moments=0, workspace=0,
                      max_seq_len=2, terminated=0, truncated=0, seq_lens=p(res[2]), seq_row=p(res[3]), seq_col=p(res[4]), reserved=[0, 0])
    res, io = one_call("seq_batch", dict(b, truncated=z(u8)), "phx_seq_batch")          # T * N with one
    assert io["capacity"] == T * N and tuple(res[1].shape) == (T * N, 2, 16)
    res, io = one_call("seq_batch", dict(a, out=None), "phx_seq_batch")
    assert_allocated(res[:8], [(i64, (N + 1,)), (i32, (5, 2, ROW_WORDS)), (i32, (5,)), (i32, (5,)), (i32, (5,)), (i32, (5, 2)), (i32, (5, 2)),
                               (u8, (32,))])
    assert io["moments"] == p(res[7]) and io["workspace"] % 16 == 0 and io["workspace"] != 0


def test_replay_add_marshalling_and_the_three_kinds_of_count():
    a = CASES["replay_add"].full
    want = dict(capacity=RING, src_capacity=5, count=0, row_words=ROW_WORDS, reserved0=0, count_ptr=p(a["count"]), src=p(a["records"]),
                ring=p(a["ring"]), state=p(a["state"]), reserved=[0, 0])
    res, io = one_call("replay_add", a, "phx_replay_add")                              # a device count: the pointer, and count = 0
    assert io == want and res is None
    b = CASES["replay_add"].bare
    _, io = one_call("replay_add", b, "phx_replay_add")                                # None: all of `records`
    assert io == dict(want, count=5, count_ptr=0, src=p(b["records"]))
    _, io = one_call("replay_add", dict(a, count=np.int64(3)), "phx_replay_add")
    assert io == dict(want, count=3, count_ptr=0)
    _, io = one_call("replay_add", dict(a, records=z(i32, 5, ROW_WORDS)[:0], count=None), "phx_replay_add")     # no record: src is NULL
    assert io == dict(want, src_capacity=0, count=0, count_ptr=0, src=0)


def test_replay_sample_marshalling():
    a = CASES["replay_sample"].full
    res, io = one_call("replay_sample", a, "phx_replay_sample")
    assert io == dict(capacity=RING, n=5, row_words=ROW_WORDS, reserved0=0, seed=7, draw=9, slot_in=p(a["slots"]), ring=p(a["ring"]),
                      state=p(a["state"]), out=p(a["out"][0]), out_slot=p(a["out"][1]), reserved=[0, 0])
    assert res[0] is a["out"][0] and res[1] is a["out"][1]
    res, io = one_call("replay_sample", dict(a, out=(a["out"][0], None)), "phx_replay_sample")
    assert io["out_slot"] == 0 and res[1] is None
    b = CASES["replay_sample"].bare
    res, io = one_call("replay_sample", b, "phx_replay_sample")
    assert_allocated(res, [(i32, (5, ROW_WORDS)), (i64, (5,))])
    assert io == dict(capacity=RING, n=5, row_words=ROW_WORDS, reserved0=0, seed=0, draw=0, slot_in=0, ring=p(b["ring"]), state=p(b["state"]),
                      out=p(res[0]), out_slot=p(res[1]), reserved=[0, 0])
