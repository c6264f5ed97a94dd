"""The stop path of the served kernels' mailbox (sparc_amd/csrc/wedm_served.h): when every environment of a block is
terminated, the block's scalar wave publishes SV_STOP | SV_DONE and the walkers leave their loop early.  The three kernels
that share the walkers' side of that protocol -- wedm_step_served (kernel 9), wedm_step_lanes_served (11) and
wedm_step_regs_served (12) -- run a batch of N = 2 EPB + 5 environments of a 128-segment wire (EPB: environments per block)
against the CPU oracle, every state block bit for bit: block 0 breaks every wire at its first step and stops, block 1 runs
with one frozen lane, the last block is partly dead."""
from __future__ import annotations

import functools

import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend

# (kernel, lanes per environment, environments per block)
CASES = [(9, 4, 48), (9, 8, 24), (11, 4, 48), (11, 8, 24), (11, 16, 12), (12, 0, 64)]
FAMILY = {9: "wedm_step_served<", 11: "wedm_step_lanes_served<", 12: "wedm_step_regs_served<"}
FUSED, SINGLE = 300, 5


def make_env(epb, **kw):
    env = WireEDMEnv(num_envs=2 * epb + 5, wire_params=WireModuleParameters(segment_len=0.625),
                     config=EnvironmentConfig(target_cutting_distance=5000.0), **kw)
    assert env.n_segments == 128
    return env


def scenario(env, epb):
    env.reset(seed=4100 + epb)
    env.state.workpiece_position = 21.0
    env.state.wire_position = 10.0
    env.state.target_position = 5000.0
    hot = env.state.wire_temperature
    hot[:epb, 64] = 1600.0       # every environment of block 0 breaks its wire at the first step: the block stops
    hot[epb + 1, 64] = 1600.0    # and one environment of block 1: a frozen lane beside live ones
    return env.make_action(0.1, 80.0, 17, 3.0, 20.0)


def run(env, epb, after_fused=lambda: None):
    act = scenario(env, epb)
    env.step_many(act, FUSED)
    after_fused()
    for _ in range(SINGLE):
        env.step(act)


@functools.lru_cache(maxsize=None)
def oracle_run(epb):
    """The CPU oracle's blocks after the run, once per block size, and what makes the run reach the stop path: exactly the
    environments of block 0 and environment EPB + 1 are broken, every other one has sparked."""
    env = make_env(epb, device="cpu", backend=OracleBackend)
    run(env, epb)
    n = env.num_envs
    expect_broken = torch.zeros(n, dtype=torch.bool)
    expect_broken[:epb] = True
    expect_broken[epb + 1] = True
    broken = env.state.is_wire_broken[:n].bool().cpu()
    assert torch.equal(broken, expect_broken), torch.nonzero(broken != expect_broken).flatten().tolist()
    sparks = env.state.spark_count[:n].cpu()
    assert int(sparks[~expect_broken].min()) >= 1, sparks.tolist()
    return env.state.clone_blocks()


@pytest.mark.parametrize("epb", sorted({c[2] for c in CASES}))
def test_the_oracle_run_stops_block_0_and_nothing_else(epb):
    """What keeps the GPU cases from passing vacuously (the conditions are asserted inside oracle_run)."""
    oracle_run(epb)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,lanes,epb", CASES)
def test_a_block_whose_environments_all_terminate_stops_and_matches_the_oracle(variant, lanes, epb):
    want = oracle_run(epb)
    gpu = make_env(epb, device="cuda:0")
    gpu.set_kernel(variant, lanes)

    def named():
        name = gpu._backend.last_kernel()
        assert name.startswith(FAMILY[variant]) and (lanes == 0 or f"<{lanes}" in name), name

    run(gpu, epb, after_fused=named)
    named()
    torch.cuda.synchronize()
    diffs = block_diffs(gpu.state.clone_blocks(), want, gpu.num_envs)
    gpu.close()
    assert not diffs, f"kernel {variant}, {lanes} lanes:\n" + "\n".join(diffs[:10])
