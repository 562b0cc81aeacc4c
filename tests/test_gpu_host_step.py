"""The three ways a step's outputs reach the host (DeviceEnv.pull_step, pull_step_lazy, pull_step_async) give the same arrays,
through HostStep.get() and HostStep.read_into() alike, and the staleness rules of the lazy and the ring-buffer results hold."""
import numpy as np
import pytest
import torch

from device_runner import DeviceRunner
from helpers import supply_chain_env
from phantom_amd.device import DeviceError

pytestmark = pytest.mark.gpu

B, S = 3, 2
NAMES = ["obs", "reward", "obs_valid", "reward_valid", "terminated", "truncated", "done_valid", "all_terminated", "all_truncated", "err"]


@pytest.fixture()
def dev():
    d = DeviceRunner(supply_chain_env(S, [3, 2], 20, B, seed=7).spec).dev
    d.reset()
    return d


def _acts(n):
    rng = np.random.default_rng(1)
    return [torch.from_numpy(rng.uniform(0, 100, (B, S)).astype(np.float32)).cuda() for _ in range(n)]


def _same(got, want):
    assert list(got) == list(want) == NAMES
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_every_way_to_the_host_gives_the_same_arrays(dev):
    dev.step(_acts(1)[0])
    base = {k: v.copy() for k, v in dev.pull_step().items()}
    assert (base["obs"].any() or base["reward"].any()) and not base["err"].any()     # a real step, not a zero buffer
    _same(dev.pull_step_lazy().get(), base)
    _same(dev.pull_step_async().get(), base)
    for pull in (dev.pull_step_lazy, dev.pull_step_async):
        dst = {k: np.full_like(v, 0x55) for k, v in base.items()}
        pull().read_into(dst)
        _same(dst, base)
    hs = dev.pull_step_async()
    assert hs.get() is hs.get()                                   # copied out once
    dst = {k: np.full_like(v, 0x55) for k, v in base.items()}
    hs.read_into(dst)                                             # ... and read_into() after get() serves those copies
    _same(dst, base)


def test_a_lazy_result_first_read_after_a_further_step_raises(dev):
    a = _acts(2)
    dev.step(a[0])
    lazy, lazy2 = dev.pull_step_lazy(), dev.pull_step_lazy()
    dev.step(a[1])
    with pytest.raises(DeviceError, match="first read after a later step"):
        lazy.get()
    with pytest.raises(DeviceError, match="first read after a later step"):
        lazy2.read_into({})


def test_a_held_async_result_outlives_the_reuse_of_its_buffer(dev):
    a = _acts(5)
    dev.step(a[0])
    base = {k: v.copy() for k, v in dev.pull_step().items()}
    held = dev.pull_step_async()
    later = None
    for x in a[1:]:                                               # four further rounds: the three pinned buffers have all been reused
        dev.step(x)
        later = dev.pull_step_async()
    _same(held.get(), base)                                       # (copied out by materialise() right before the reuse)
    _same(later.get(), {k: v.copy() for k, v in dev.pull_step().items()})
    assert any(held.get()[k].tobytes() != later.get()[k].tobytes() for k in ("obs", "reward"))
