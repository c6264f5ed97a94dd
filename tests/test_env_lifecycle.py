"""The environment's launch lifecycle (sparc_amd/csrc/wedm_lifecycle.h and the kernels' own openings: open with the
in-launch autoreset, end of a microsecond, close with reward and clock) on the kernels and lane counts that
tests/test_gpu_parity.py::test_in_kernel_autoreset_and_reward_match_oracle_and_host_path leaves out.  Same body, same
assertions, on a batch small enough for every case: 96 environments (with one lane per environment most of a block is dead
lanes, with 16 lanes six blocks) of a 128-segment wire, which the register kernels 7, 8 and 12 accept."""
from __future__ import annotations

import functools

import pytest
import torch

from sparc_amd import WireEDMVectorEnv, WireModuleParameters
from tests._compare import assert_blocks_equal
from tests._oracle_backend import OracleBackend
from tests.test_gpu_parity import KERNELS, SERVED, SERVED_ANY
from tests.test_next_rows import terminating_pair

N, INTERVALS = 96, 5
ACTION = (0.05, 80.0, 13, 2.0, 20.0)
COVERED = [(0, 0), (2, 4), (3, 8), (4, 4), (1, 0), (5, 0), (6, 8), (9, 8), (9, 4), (11, 8)]  # the parity test's own list
CASES = [kl for kl in KERNELS + SERVED + SERVED_ANY + [(7, 1), (7, 2), (8, 4), (8, 16), (10, 4), (12, 0)] if kl not in COVERED]
# the family each forced kernel number runs (a forced kernel that fell back to another one would pass the parity unnoticed)
FAMILY = {2: "wedm_step_lanes_pk<", 3: "wedm_step_fused<", 4: "wedm_step_packed<", 6: "wedm_step_stream<", 7: "wedm_step_regs<",
          8: "wedm_step_regs_wide<", 10: "wedm_step_lanes<", 11: "wedm_step_lanes_served<", 12: "wedm_step_regs_served<"}


def wire128():
    return dict(wire_params=WireModuleParameters(segment_len=0.625))


@functools.lru_cache(maxsize=None)
def oracle_intervals():
    """The CPU oracle with the in-launch reset, once for every case: (reward, terminated, blocks) after each interval."""
    env, _ = terminating_pair(N, OracleBackend, **wire128())
    vec = WireEDMVectorEnv(env)
    act = env.make_action(*ACTION)
    out = []
    for _ in range(INTERVALS):
        _, r, t, _, _ = vec.step(act)
        out.append((r.clone(), t.clone(), env.state.clone_blocks()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,lanes", CASES)
def test_in_kernel_autoreset_and_reward_on_the_remaining_kernels(variant, lanes):
    a, b = terminating_pair(N, None, device="cuda:0", **wire128())
    a.set_kernel(variant, lanes), b.set_kernel(variant, lanes)
    va, vb = WireEDMVectorEnv(a), WireEDMVectorEnv(b, reward="progress")
    act_a, act_b = a.make_action(*ACTION), b.make_action(*ACTION)
    most = 0.0
    for k, (rc, tc, Cc) in enumerate(oracle_intervals()):
        oa, ra, ta, ua, ia = va.step(act_a)
        ob, rb, tb, ub, ib = vb.step(act_b)
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(ta.cpu(), tc), k
        assert torch.equal(ra, rb) and torch.equal(ra.cpu(), rc), k
        A, B = a.state.clone_blocks(), b.state.clone_blocks()
        assert_blocks_equal(A, Cc, N)                                  # GPU == oracle, reward row included
        assert_blocks_equal(A, B, N, skip_rows=("reward",))            # in-kernel reset == host-driven reset
        most = max(most, float(ta.float().mean()))
        assert a._backend.last_kernel().startswith(FAMILY[variant]), a._backend.last_kernel()
    assert most >= 0.3 and int(a.state.episode.max()) >= 1
    assert va._in_kernel_reset and not vb._in_kernel_reset
