"""Fuzz of the kernels' ENVP and PULSE forms against the CPU oracle (tests/_oracle_backend.py, OracleBackendRows), on
every byte after every launch: the state blocks, the observation, the reward, the pulse rows and the crater log.

Modelled on `_fuzz_case` in tests/test_gpu_parity.py (ragged batch sizes, wire lengths, ``dt``, ``servo_interval``,
control mode, per-environment geometry, extreme gaps and debris, autoreset with a crater log, the reference-compatible
modes, random shorts, launches of 1 / 7 / 400 / 1300 us) with every one of the 15 randomisable physics parameters drawn
per environment (tests/_envp_draw.py: both sides of each edge of the model inside one wave).  Some cases change the rows
between launches from device tensors (the device-side derivation, ``omega_n`` with 26 significant bits), some bind a trace
(kernel 1's TRACE + ENVP form), some count pulses (kernel 1's PULSE + ENVP form), some type the stencil in float64.
A quarter of the cases keep uniform parameters and count pulses on every kernel with a PULSE form.

``WEDM_FUZZ_ENVP_CASES`` sets the number of cases (default 96, about ten seconds)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from sparc_amd import (DielectricModuleParameters, EnvironmentConfig, IgnitionModuleParameters, MaterialModuleParameters,
                       MechanicsModuleParameters, WireEDMEnv, WireModuleParameters, _abi)
from sparc_amd._lib import WedmError
from tests import _envp_draw as D
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackendRows

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("WEDM_FUZZ_ENVP_CASES", "96"))
ENVP_KERNELS = [(0, 0), (1, 0), (2, 1), (2, 2), (2, 4), (2, 8), (2, 16)]


def _config_kw(rng, case, n, *, per_env):
    u = rng.uniform
    kw = dict(
        mechanics_control_mode="velocity" if case % 5 in (1, 4) else "position",
        config=EnvironmentConfig(workpiece_height=float(u(8, 32)), wire_diameter=float(rng.choice([0.1, 0.2, 0.3])),
                                 dt=int(rng.choice([1, 2])), servo_interval=int(rng.choice([200, 500, 1000])),
                                 initial_gap=float(u(15, 40)), target_cutting_distance=5000.0),
        ignition_params=IgnitionModuleParameters(
            base_critical_density=float(u(0.05, 0.4)), gap_coefficient=float(u(0.005, 0.03)),
            sigmoid_steepness=float(rng.choice([50.0, 500.0])), hard_short_gap=float(u(1, 4)),
            debris_short_duration=int(rng.integers(10, 80)), random_short_duration=int(rng.integers(20, 120)),
            random_short_max_probability=float(rng.choice([0.0, 0.003, 0.01])), spark_voltage_factor=float(u(0.2, 0.5)),
            ignition_c_coeff=float(14.05 * u(0.9, 1.3))),
        wire_params=WireModuleParameters(segment_len=float(rng.choice([0.2, 0.25, 0.5, 0.625])),
                                         buffer_len_bottom=float(u(10, 40)), buffer_len_top=float(u(10, 40)),
                                         base_convection_coefficient=float(u(8000, 20000)),
                                         plasma_efficiency=float(u(0.05, 0.3)), critical_temp_threshold=float(u(0.7, 0.95))),
        material_params=MaterialModuleParameters(base_overcut=float(u(0.08, 0.2))),
        dielectric_params=DielectricModuleParameters(base_flow_rate=float(u(50, 200)), debris_obstruction_coeff=float(u(0.5, 3)),
                                                     reference_gap=float(u(15, 40)), dielectric_temperature=float(u(285, 300))),
        mechanics_params=MechanicsModuleParameters(omega_n=float(u(150, 400)), zeta=float(u(0.2, 0.9)),
                                                   max_speed=float(3e4 * u(0.3, 1.5))),
    )
    if per_env:
        kw["workpiece_height"] = rng.uniform(8, 32, n)
        kw["wire_diameter"] = rng.choice([0.1, 0.15, 0.25], n)
    return kw


def _compare(gpu, cpu, n, where):
    g, c = gpu.state.clone_blocks(), cpu.state.clone_blocks()
    diffs = block_diffs(g, c, n)
    assert not diffs, f"{where}:\n" + "\n".join(diffs[:12])
    if "pulse" in c:
        bad = torch.nonzero((g["pulse"][:, :n] != c["pulse"][:, :n]).any(dim=0)).flatten()
        assert bad.numel() == 0, f"{where}: pulse rows differ for {bad.numel()} envs; env {int(bad[0])}: got " \
            f"{g['pulse'][:, int(bad[0])].tolist()} want {c['pulse'][:, int(bad[0])].tolist()}"
    if "crater_log" in c:
        G, C = g["crater_log"][:, :n], c["crater_log"][:, :n]
        filled = torch.arange(G.shape[0])[:, None] < g["i32"][_abi.I32.SPARK_COUNT, :n][None, :]
        assert torch.equal(torch.where(filled, G, 0), torch.where(filled, C, 0)), f"{where}: crater log differs"
    return g


def _fuzz(case):
    rng = np.random.default_rng(77000 + case)
    pulse_only = case % 4 == 3   # uniform parameters, every kernel with a PULSE form
    n = int(rng.choice([65, 128, 200, 333]))
    per_env = case % 3 == 2
    kw = _config_kw(rng, case, n, per_env=per_env)
    extreme = case % 2 == 1 or case >= 8
    trace = not pulse_only and case % 6 == 4
    if extreme and not trace:   # terminations: reset inside the launch, kernel-side reward, crater log
        kw.update(autoreset=True, reward="progress", crater_log_capacity=8)
    compat = case % 5 in (2, 3)
    if compat:
        kw.update(reset_semantics="reference", freeze_terminated=(case % 5 == 2))
    f64 = not pulse_only and case % 7 == 5
    if f64:
        kw["stencil_dtype"] = "float64"
    pulse = pulse_only or case % 4 == 1
    if pulse:
        kw["pulse_stats"] = True
    values = None
    if not pulse_only:
        values = D.draw(rng, n)
        D.spread_ok(values)
        kw["env_params"] = values
    gpu = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
    cpu = WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackendRows, **kw)
    seed = int(rng.integers(1, 1 << 40))
    gaps, debris = rng.uniform(6, 30, n), rng.uniform(0, 0.01, n)
    if extreme:
        gaps = np.where(rng.random(n) < 0.5, rng.uniform(0.5, 5, n), rng.uniform(5, 15, n))
        debris = np.where(rng.random(n) < 0.3, rng.uniform(0, 0.2, n), debris)
    target = np.where(np.arange(n) % 7 == 3, 10.0 + gaps + 0.001, 5000.0) if extreme else np.full(n, 5000.0)
    for env in (gpu, cpu):
        env.reset(seed=seed)
        env.state.wire_position = 10.0
        env.state.workpiece_position = torch.as_tensor(10.0 + gaps)
        env.state.target_position = torch.as_tensor(target)
        env.state.debris_volume = torch.as_tensor(debris)
    if trace:
        for env in (gpu, cpu):
            env.bind_trace(["current", "voltage", "wire_position"], every=int(rng.choice([7, 250])), capacity=16)
    S = gpu.n_segments
    if pulse_only:
        kernels = [(0, 0), (1, 0), (2, 0), (2, 4), (2, 8)]
        if not per_env:   # (the register kernels take uniform geometry only; kernel 7 wires of at most 128 segments)
            kernels += [(8, 0), (8, 16)] + ([(7, 0), (7, 1)] if S <= 128 else [])
    else:
        kernels = list(ENVP_KERNELS)
    drawn = [kernels[i] for i in rng.permutation(len(kernels))[:5]]
    velocity = kw["mechanics_control_mode"] == "velocity"
    servo = rng.uniform(50, 300, n) if velocity else rng.uniform(-0.05, 0.3, n)
    if extreme:
        servo = servo * rng.choice([1.0, 1.0, 20.0, -3.0], n)
    modes = rng.choice([15, 17] if extreme else [1, 3, 5, 7, 9, 11, 13, 15, 17], n).astype(np.int32)
    volt, on, off = float(rng.uniform(60, 120)), float(rng.choice([1.5, 2.0, 3.0])), float(rng.uniform(10, 60))
    acts = [env.make_action(servo, volt, modes, on, off) for env in (gpu, cpu)]
    update_at = int(rng.integers(1, 4)) if (values is not None and case % 3 != 1) else -1
    ran, sparks = 0, 0
    for i, (variant, lanes) in enumerate(drawn + [(0, 0)]):
        if i == len(drawn) and ran >= 2:   # (one more launch on the automatic plan where the draws found too few that fit)
            break
        if i == update_at:   # new rows for a masked part of the batch, from device tensors (the device-side derivation)
            new = D.draw(rng, n)
            new["omega_n"] = D.omega_26bit(new["omega_n"])
            names = [m for m in D.envp.NAMES if rng.random() < 0.7] or ["omega_n"]
            mask = rng.random(n) < 0.5
            gpu.set_env_params({m: torch.from_numpy(new[m]).to("cuda:0") for m in names},
                               mask=torch.from_numpy(mask).to("cuda:0"))
            cpu.set_env_params({m: new[m] for m in names}, mask=mask)
            torch.cuda.synchronize()
            assert torch.equal(gpu._envp_rows.cpu(), cpu._envp_rows), "device-derived rows differ from the host's"
        gpu.set_kernel(variant, lanes)
        k = int(rng.choice([1, 7, 400, 1300]))
        samples = gpu._backend.trace_samples() if trace else 0
        try:
            gpu.step_many(acts[0], k)
        except WedmError as exc:   # a lane count whose chunks do not fit in LDS, or a form the launch does not have
            assert "UNSUPPORTED" in str(exc) or "LDS" in str(exc), exc
            continue
        cpu.step_many(acts[1], k)
        torch.cuda.synchronize()
        name = gpu._backend.last_kernel()
        where = f"case {case}: kernel {name} ({variant},{lanes}) after {k} us (n={n}, S={S}, dt={gpu.dt}, " \
                f"servo={gpu.servo_interval}, {kw['mechanics_control_mode']})"
        assert ("[envp]" in name) == (values is not None), where
        assert ("[pulse]" in name) == pulse, where
        assert not f64 or "[f64 stencil]" in name, where
        if trace and gpu._backend.trace_samples() > samples:   # (a launch without a sample in it keeps its kernel)
            assert "wedm_step_global" in name, where
        g = _compare(gpu, cpu, n, where)
        sparks = max(sparks, int(g["i32"][_abi.I32.SPARK_COUNT, :n].sum()) + int(g["i32"][_abi.I32.EPISODE, :n].sum()))
        ran += 1
        if compat and ran == 2:   # a second episode for a third of the environments
            for env in (gpu, cpu):
                env.reset(seed=seed + 1, options={"mask": np.arange(n) % 3 == case % 3})
                wp = env.state.workpiece_position.cpu().numpy()
                env.state.wire_position = torch.as_tensor(np.where(np.arange(n) % 3 == case % 3, wp - gaps,
                                                                   env.state.wire_position.cpu().numpy()))
    assert ran >= 2, f"case {case}: only {ran} launches ran"
    assert sparks > 0, f"case {case}: nothing sparked"
    if values is not None:   # the batch really held different physics
        rows = gpu._envp_rows[:, :n].cpu()
        assert all(len(torch.unique(rows[r])) >= 2 for r in range(_abi.ENVP_COUNT))


@pytest.mark.parametrize("case", range(CASES))
def test_env_params_and_pulse_forms_match_the_oracle(case):
    _fuzz(case)
