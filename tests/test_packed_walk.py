"""Both includers of the shared packed walk (sparc_amd/csrc/wedm_packed_walk.inc) -- wedm_step_packed (kernel 4) and the walkers
of wedm_step_served (kernel 9) -- through the tile-geometry sweep of tests/test_gpu_parity.py, bit-exact against the CPU oracle
on a real MI355X."""
from __future__ import annotations

import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

SWEEP_N = list(range(9, 171))
# (kernel, lanes per environment) and the family's name in last_kernel(); blocks of 64, 32, 48 and 24 environments
FORCED = [(4, 4, "wedm_step_packed<4>"), (4, 8, "wedm_step_packed<8>"), (9, 4, "wedm_step_served<4>"), (9, 8, "wedm_step_served<8>")]
# (length, kernel) pairs the library may refuse: 0.  Both kernels refuse only a wire whose two chunks per lane do not fit: no
# walk table for 2 L chunks, or an LDS image beyond the limit.  Up to 170 segments over 8 or 16 chunks a chunk has at most
# ceil(170 / 8) = 22 cells: every table builds (the limit is 159 cells) and the image is at most 2 x 22 + 2 = 46 rows of 1 KiB
# (+ the served kernel's mailbox), below the 64 KiB every device grants.  So every one of the 162 x 4 pairs has to run.
MAX_REFUSED = 0


@pytest.mark.parametrize("n_lo", SWEEP_N[::18])
def test_packed_walk_sweep_every_wire_length_packed_and_served(n_lo):
    """Every wire length from 9 to 170 segments x {packed, served} x {4, 8} lanes per environment against the oracle: the
    scenario of test_tile_geometry_sweep_every_wire_length_every_lane_count (chunk lengths, tails of 1..7 cells, chunks wholly
    past the end, zone / contact boundaries at every tile offset; sparks, current, a wire break and hot end cells in the
    batch), on 100 environments, so that every kernel's last block is partly dead (100 mod 64, 32, 48, 24 != 0)."""
    from sparc_amd._lib import WedmError

    n_envs, ran, refused = 100, 0, []
    for n_seg in SWEEP_N[SWEEP_N.index(n_lo): SWEEP_N.index(n_lo) + 18]:
        kw = dict(wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                  config=EnvironmentConfig(target_cutting_distance=5000.0))

        def scenario(env):
            env.reset(seed=1000 + n_seg)
            env.state.workpiece_position = 21.0
            env.state.wire_position = 10.0
            env.state.target_position = 5000.0
            hot = env.state.wire_temperature
            hot[5, n_seg // 2] = 1600.0       # environment 5 breaks its wire at the first step: a frozen lane in its wave
            hot[70, n_seg - 1] = 900.0        # (in a wave without a frozen lane:) a hot last cell (Neumann end) ...
            hot[71, 1] = 900.0                # ... and a hot first interior cell
            return env.make_action(0.1, 80.0, 17, 3.0, 20.0)

        # the oracle's half first, on the CPU, once per length
        cpu = WireEDMEnv(num_envs=n_envs, device="cpu", backend=OracleBackend, **kw)
        assert cpu.n_segments == n_seg
        act = scenario(cpu)
        cpu.step_many(act, 290)
        for _ in range(10):
            cpu.step(act)
        want = cpu.state.clone_blocks()
        assert int(cpu.state.spark_count.sum()) > n_envs and bool(cpu.state.is_wire_broken[5])

        gpu = WireEDMEnv(num_envs=n_envs, device="cuda:0", **kw)
        for variant, lanes, family in FORCED:
            act = scenario(gpu)
            gpu.set_kernel(variant, lanes)
            try:
                gpu.step_many(act, 290)
                assert family in gpu._backend.last_kernel(), (n_seg, family, gpu._backend.last_kernel())
                for _ in range(10):
                    gpu.step(act)
                assert family in gpu._backend.last_kernel(), (n_seg, family, gpu._backend.last_kernel())
            except WedmError as exc:
                assert "UNSUPPORTED" in str(exc)
                refused.append((n_seg, family))
                continue
            torch.cuda.synchronize()
            diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
            assert not diffs, f"n_seg {n_seg}, kernel {gpu._backend.last_kernel()}:\n" + "\n".join(diffs[:10])
            ran += 1
        gpu.close()
    print(f"packed walk sweep from {n_lo}: ran {ran}, refused {refused}")
    assert len(refused) <= MAX_REFUSED and ran == 18 * len(FORCED) - len(refused), (ran, refused)
