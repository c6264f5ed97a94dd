"""The form-dependent line of the opening (sparc_amd/csrc/wedm_lifecycle.h, WEDM_ENV_RESET): the in-launch autoreset clears
the pulse block's rows in the PULSE forms of kernels 2, 7 and 8 as well.  The only other pulse-statistics autoreset test
(tests/test_pulse_stats.py) resets in a launch of one microsecond, which runs kernel 1.  In the shape of
tests/test_env_lifecycle.py: 96 environments of a 128-segment wire -- the smallest batch every register kernel accepts and
that fills and half-fills blocks -- stepped through whole control intervals against the CPU oracle."""
from __future__ import annotations

import functools

import pytest
import torch

from sparc_amd import WireEDMVectorEnv, WireModuleParameters
from tests._compare import assert_blocks_equal
from tests._oracle_backend import OracleBackendRows
from tests.test_next_rows import terminating_pair

N, INTERVALS = 96, 6
ACTION = (0.05, 80.0, 13, 2.0, 20.0)
CASES = [(1, 0), (2, 4), (7, 1), (7, 2), (8, 4), (8, 16)]
FAMILY = {1: "wedm_step_global[", 2: "wedm_step_lanes_pk<", 7: "wedm_step_regs<", 8: "wedm_step_regs_wide<"}


def pulse_batch(backend, device="cpu"):
    """The batch that resets inside its launches (the first of terminating_pair's two), with the pulse block bound."""
    return terminating_pair(N, backend, device=device, pulse_stats=True, wire_params=WireModuleParameters(segment_len=0.625))[0]


@functools.lru_cache(maxsize=None)
def oracle_intervals():
    """The CPU oracle (OracleBackendRows: the plain one refuses pulse_stats), once for every case.  Per interval: the state
    blocks and the six pulse rows after it, and which environments its launch reset while their pulse rows held counts."""
    env = pulse_batch(OracleBackendRows)
    vec = WireEDMVectorEnv(env)
    act = env.make_action(*ACTION)
    out = []
    for _ in range(INTERVALS):
        counted = env.state.pulse[:, :N].abs().sum(dim=0) > 0
        episode = env.state.episode[:N].clone()
        vec.step(act)
        reset_with_counts = (env.state.episode[:N] > episode) & counted
        out.append((env.state.clone_blocks(), env.state.pulse[:, :N].clone(), reset_with_counts))
    return out


def test_the_oracle_run_resets_environments_whose_pulse_rows_hold_counts():
    """What keeps the GPU cases from passing vacuously: launches that reset environments with non-zero pulse rows."""
    per_interval = [int(r.sum()) for _, _, r in oracle_intervals()]
    assert per_interval[0] == 0 and sum(1 for c in per_interval if c >= 1) >= 2, per_interval


@pytest.mark.gpu
@pytest.mark.parametrize("variant,lanes", CASES)
def test_in_launch_autoreset_clears_the_pulse_rows_in_every_pulse_form(variant, lanes):
    env = pulse_batch(None, device="cuda:0")
    env.set_kernel(variant, lanes)
    vec = WireEDMVectorEnv(env)
    act = env.make_action(*ACTION)
    resets = [int(r.sum()) for _, _, r in oracle_intervals()]
    assert sum(1 for c in resets if c >= 1) >= 2, resets
    for k, (blocks, pulse, _) in enumerate(oracle_intervals()):
        vec.step(act)
        torch.cuda.synchronize()
        assert_blocks_equal(env.state.clone_blocks(), blocks, N)
        assert torch.equal(env.state.pulse[:, :N].cpu(), pulse), k
        name = env._backend.last_kernel()
        assert name.startswith(FAMILY[variant]) and "[pulse]" in name, name
    assert vec._in_kernel_reset
