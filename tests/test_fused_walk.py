"""Both includers of the shared one-chunk LDS tile walk (sparc_amd/csrc/wedm_fused_walk.inc) -- wedm_step_fused (kernel 3) and the
LDS walk of wedm_step_stream (kernel 6) -- through the tile-geometry sweep of tests/test_gpu_parity.py, in the handle modes that
sweep does not fix, bit-exact against the CPU oracle on a real MI355X."""
from __future__ import annotations

import pytest
import torch

from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

SWEEP_N = list(range(9, 171))
# Handle modes.  Autoreset puts wedm_step_fused on its F_FROZEN_OK forms (the tile code's copy in which frozen lanes do not
# store) and both kernels through the in-launch reinitialisation of the wire; the float64 typing with autoreset runs
# F_FROZEN_OK | F_F64 on wedm_step_fused and F_ONE | F_F64 on wedm_step_stream.
MODES = {
    "f32": dict(),
    "f32_autoreset": dict(autoreset=True),
    "f64_autoreset": dict(stencil_dtype="float64", autoreset=True),
}
# Lanes per environment (blocks of 128, 64, 32 and 16 environments).  No (length, kernel, lanes) may be refused: a chunk has at
# most ceil(170 / 2) = 85 cells, 88 after the stream table's rounding to whole words -- below the walk table's 159 and the
# stream kernel's 104 -- and its image of at most 89 rows of 1 KiB is below the MI355X's 160 KiB.  In the float64 typing the
# stream kernel takes chunks of at most 64 cells: from 4 lanes up, ceil(170 / 4) -> 44.  (One lane per environment, which does
# refuse long wires, stays with test_tile_geometry_sweep_every_wire_length_every_lane_count.)
LANES = {"f32": (2, 4, 8, 16), "f32_autoreset": (2, 4, 8, 16), "f64_autoreset": (4, 8, 16)}
FUSED, STREAM = 3, 6


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_lo", SWEEP_N[::18])
def test_fused_walk_sweep_every_wire_length_fused_and_stream(n_lo, mode):
    """Every wire length from 9 to 170 segments x {fused, stream} x lanes per environment against the oracle: the scenario of
    test_tile_geometry_sweep_every_wire_length_every_lane_count (chunk lengths, tails of 1..7 cells, chunks wholly past the end,
    zone / contact boundaries at every tile offset; sparks, current, a wire break and hot end cells in the batch), one launch of
    290 us and ten of 1 us, on 100 environments, so that every kernel's last block is partly dead (100 mod 128, 64, 32, 16 != 0).
    In the float64 typing a forced kernel 6 runs single microseconds only: there the 290 us run on kernel 3 at the same lanes
    and the ten single steps on kernel 6."""
    f64, autoreset = "stencil_dtype" in MODES[mode], "autoreset" in MODES[mode]
    tag = "[f64 stencil]" if f64 else ""
    n_envs, ran = 100, 0
    for n_seg in SWEEP_N[SWEEP_N.index(n_lo): SWEEP_N.index(n_lo) + 18]:
        kw = dict(wire_params=WireModuleParameters(segment_len=80.0 / (n_seg + 0.5)),
                  config=EnvironmentConfig(target_cutting_distance=5000.0), **MODES[mode])

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

        # the oracle's half first, on the CPU, once per (length, mode)
        cpu = WireEDMEnv(num_envs=n_envs, device="cpu", backend=OracleBackend, **kw)
        assert cpu.n_segments == n_seg
        act = scenario(cpu)
        cpu.step_many(act, 290)
        assert bool(cpu.state.is_wire_broken[5])
        for _ in range(10):
            cpu.step(act)
        want = cpu.state.clone_blocks()
        assert int(cpu.state.spark_count.sum()) > 100
        # (next-step autoreset: the first single step starts environment 5's second episode)
        assert (int(cpu.state.episode[5]), bool(cpu.state.is_wire_broken[5])) == ((1, False) if autoreset else (0, True))

        gpu = WireEDMEnv(num_envs=n_envs, device="cuda:0", **kw)
        for variant in (FUSED, STREAM):
            for lanes in LANES[mode]:
                long_variant = FUSED if f64 else variant
                names = {FUSED: f"wedm_step_fused<{lanes}>", STREAM: f"wedm_step_stream<{lanes}>"}
                act = scenario(gpu)
                gpu.set_kernel(long_variant, lanes)
                gpu.step_many(act, 290)
                name = gpu._backend.last_kernel()
                assert names[long_variant] in name and tag in name, (n_seg, names[long_variant], name)
                gpu.set_kernel(variant, lanes)
                for _ in range(10):
                    gpu.step(act)
                name = gpu._backend.last_kernel()
                assert names[variant] in name and tag in name, (n_seg, names[variant], name)
                torch.cuda.synchronize()
                diffs = block_diffs(gpu.state.clone_blocks(), want, n_envs)
                assert not diffs, f"n_seg {n_seg}, kernel {name}:\n" + "\n".join(diffs[:10])
                ran += 1
        gpu.close()
    print(f"fused walk sweep from {n_lo}, {mode}: ran {ran}")
    assert ran == 18 * 2 * len(LANES[mode]), ran
