"""GPU: phx_create / phx_destroy hand back every device allocation a handle made, on each of the four plan families
phx_create builds (plain supply chain, FSM supply chain, Stackelberg market, digital ads)."""
import ctypes as C

import pytest

import phantom_amd as ph
from phantom_amd import _abi
from helpers import market_env, supply_chain_env

pytestmark = pytest.mark.gpu

PARENT_DRIFT_BYTES = 0       # what a balanced pair leaves: every hipMalloc of a handle has its hipFree in phx_destroy (figure of the library before the split: see the test)


def _tiny_envs(B=8):
    return {
        "plain supply chain": supply_chain_env(3, [2] * 3, 10, B, seed=1),
        "FSM supply chain": supply_chain_env(3, [2] * 3, 10, B, fsm=True, seed=1),
        "2x3 market": market_env(2, 3, 2, 6, B, seed=1),
        "ads": ph.DigitalAdsEnv(num_steps=6, num_agents_theme={"travel": 2, "tech": 2}, batch_size=B, seed=3,
                                agent_supertypes={f"ADV_{i + 1}": ph.AdvertiserAgent.Supertype(budget=0.3) for i in range(4)}),
    }


def test_create_destroy_is_balanced():
    """After two warm-up cycles, 30 create / destroy cycles per env over ONE caller-owned state blob: the device's free memory
    after cycle 30 is what it was after cycle 3.  The bound is 0 bytes: the handle's allocations are hipMalloc / hipFree pairs and the
    runtime's own lazy allocations (code objects, the NULL stream's pools) fall into the warm-up cycles.  The figure of the library before
    phx_create was split into stages has not been measured; 0 is the expected one.
    A handle that leaks a table or an early return that skips phx_destroy shows as a positive drift."""
    import torch
    lib = _abi.load_library()
    dev = torch.cuda.current_device()
    for name, env in _tiny_envs().items():
        cs, keep = env.spec.to_ctypes()
        nbytes = lib.phx_state_nbytes(C.byref(cs))
        assert nbytes > 0, name
        state = torch.zeros(int(nbytes), dtype=torch.uint8, device=f"cuda:{dev}")
        torch.cuda.synchronize()

        def cycle():
            h = C.c_void_p()
            rc = lib.phx_create(C.byref(cs), dev, state.data_ptr(), nbytes, C.byref(h))
            assert rc == 0, (name, lib.phx_last_error())
            lib.phx_destroy(h)

        cycle(); cycle()
        free = {}
        for n in range(1, 31):
            cycle()
            if n in (3, 30):
                free[n] = torch.cuda.mem_get_info(dev)[0]
        drift = free[3] - free[30]
        print(f"create/destroy drift, {name}: {drift} bytes")
        assert drift <= PARENT_DRIFT_BYTES, name
