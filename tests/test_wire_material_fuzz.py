"""Fuzz of the kernels' MAT forms (per-environment wire material, wedm_bind_wire_material) against the CPU oracle
(tests/_oracle_backend.py, OracleBackendRows), on every byte after every launch: the state blocks, the observation, the
reward, the pulse rows and the filled crater-log slots.

Each case draws 2 to 5 materials around brass and copper (tests/_wmat_draw.py), at least one whose float32 critical
temperature rounds up and one where it rounds down, and assigns them to the environments at random, with per-environment
geometry; hot bands sit between each environment's own critical and breaking temperatures and on the float32 neighbours
of both.  Per case: per-environment physics parameters on or off, pulse statistics on or off, a trace sample, the float64
stencil, autoreset with a crater log or the reference-compatible modes, launches of 1 / 7 / 400 / 1300 us, and in some
cases a masked `set_wire_material` from device tensors between launches.  Kernels (0,0), (1,0) and (2,L) for L = 1..16.

``WEDM_FUZZ_WMAT_CASES`` sets the number of cases (default 128, about ten seconds)."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest
import torch

from sparc_amd import WireEDMEnv, _abi
from sparc_amd._lib import WedmError
from tests import _envp_draw as D
from tests import _wmat_draw as W
from tests._oracle_backend import OracleBackendRows
from tests.test_env_params_fuzz import _compare, _config_kw

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("WEDM_FUZZ_WMAT_CASES", "128"))
WMAT_KERNELS = [(0, 0), (1, 0), (2, 1), (2, 2), (2, 4), (2, 8), (2, 16)]
BAND = slice(30, 36)  # on the wire for every height and segment length drawn (at least 44 segments)


def _materials(rng, case, threshold):
    k = int(rng.integers(2, 6))
    dirs = [(+1, int(rng.choice([-1, 1]))), (-1, int(rng.choice([-1, 1])))] + \
        [(int(rng.choice([-1, 1])), int(rng.choice([-1, 1]))) for _ in range(k - 2)]
    mats = [W.draw_material(rng, f"fuzz_{case}_{i}", c, b, threshold) for i, (c, b) in enumerate(dirs)]
    if rng.random() < 0.5:   # a built-in or fixture material among them
        mats[-1] = W.BRASS if rng.random() < 0.5 else W.COPPER
    W.register(mats)
    return mats


def _fuzz(case):
    rng = np.random.default_rng(91000 + case)
    n = int(rng.choice([65, 128, 200, 333]))
    kw = _config_kw(rng, case, n, per_env=True)
    threshold = float(kw["wire_params"].critical_temp_threshold)
    mats = _materials(rng, case, threshold)
    names = [m.name for m in mats]
    index = rng.integers(0, len(mats), n)
    index[: len(mats)] = np.arange(len(mats))
    rng.shuffle(index)
    kw.update(wire_material=[names[i] for i in index], wire_material_table=names)
    kw["config"] = dataclasses.replace(kw["config"], wire_material=names[int(rng.integers(0, len(mats)))])
    extreme = case % 2 == 1
    trace = case % 6 == 4
    if extreme and not trace:
        kw.update(autoreset=True, reward="progress", crater_log_capacity=8)
    compat = case % 5 in (2, 3)
    if compat:
        kw.update(reset_semantics="reference", freeze_terminated=(case % 5 == 2))
    f64 = case % 7 == 5
    if f64:
        kw["stencil_dtype"] = "float64"
    pulse = case % 4 == 1
    if pulse:
        kw["pulse_stats"] = True
    envp = case % 3 == 0
    if envp:
        values = D.draw(rng, n)
        kw["env_params"] = values
    gpu = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
    cpu = WireEDMEnv(num_envs=n, device="cpu", backend=OracleBackendRows, **kw)
    seed = int(rng.integers(1, 1 << 40))
    gaps, debris = rng.uniform(6, 30, n), rng.uniform(0, 0.01, n)
    if extreme:
        gaps = np.where(rng.random(n) < 0.5, rng.uniform(0.5, 5, n), rng.uniform(5, 15, n))
        debris = np.where(rng.random(n) < 0.3, rng.uniform(0, 0.2, n), debris)
    target = np.where(np.arange(n) % 7 == 3, 10.0 + gaps + 0.001, 5000.0) if extreme else np.full(n, 5000.0)
    tc, tb = W.limits(mats, index, threshold)
    band = torch.from_numpy(W.hot_bands(rng, tc, tb))
    for env in (gpu, cpu):
        env.reset(seed=seed)
        env.state.wire_position = 10.0
        env.state.workpiece_position = torch.as_tensor(10.0 + gaps)
        env.state.target_position = torch.as_tensor(target)
        env.state.debris_volume = torch.as_tensor(debris)
        T = env.state.wire_temperature
        T[:, BAND] = band.to(env.device)[:, None].expand(-1, BAND.stop - BAND.start)
    if trace:
        for env in (gpu, cpu):
            env.bind_trace(["current", "wire_max_temperature"], every=int(rng.choice([7, 250])), capacity=16)
    drawn = [WMAT_KERNELS[i] for i in rng.permutation(len(WMAT_KERNELS))[:5]]
    velocity = kw["mechanics_control_mode"] == "velocity"
    servo = rng.uniform(50, 300, n) if velocity else rng.uniform(-0.05, 0.3, n)
    if extreme:
        servo = servo * rng.choice([1.0, 1.0, 20.0, -3.0], n)
    modes = rng.choice([15, 17] if extreme else [1, 3, 5, 7, 9, 11, 13, 15, 17], n).astype(np.int32)
    volt, on, off = float(rng.uniform(60, 120)), float(rng.choice([1.5, 2.0, 3.0])), float(rng.uniform(10, 60))
    acts = [env.make_action(servo, volt, modes, on, off) for env in (gpu, cpu)]
    switch_at = int(rng.integers(1, 4)) if case % 3 != 1 else -1
    ran = 0
    for i, (variant, lanes) in enumerate(drawn + [(0, 0)]):
        if i == len(drawn) and ran >= 2:
            break
        if i == switch_at:   # a masked switch, from device tensors (the device-side select)
            new = rng.integers(0, len(mats), n)
            mask = rng.random(n) < 0.5
            gpu.set_wire_material(torch.from_numpy(new).to("cuda:0"), mask=torch.from_numpy(mask).to("cuda:0"))
            cpu.set_wire_material(new, mask=mask)
            torch.cuda.synchronize()
            assert torch.equal(gpu._wmat_rows.cpu(), cpu._wmat_rows), "device-selected rows differ from the host's"
            assert torch.equal(gpu._geom_f64.cpu(), cpu._geom_f64)
        gpu.set_kernel(variant, lanes)
        k = int(rng.choice([1, 7, 400, 1300]))
        try:
            gpu.step_many(acts[0], k)
        except WedmError as exc:   # a lane count whose chunks do not fit in LDS, or a form the launch does not have
            assert "UNSUPPORTED" in str(exc) or "LDS" in str(exc), exc
            continue
        cpu.step_many(acts[1], k)
        torch.cuda.synchronize()
        name = gpu._backend.last_kernel()
        where = f"case {case}: kernel {name} ({variant},{lanes}) after {k} us (n={n}, S={gpu.n_segments}, " \
                f"materials={len(mats)}, dt={gpu.dt}, {kw['mechanics_control_mode']})"
        assert "[wmat]" in name, where
        assert ("[envp]" in name) == envp, where
        assert ("[pulse]" in name) == pulse, where
        assert not f64 or "[f64 stencil]" in name, where
        _compare(gpu, cpu, n, where)
        ran += 1
        if compat and ran == 2:   # a second episode for a third of the environments
            for env in (gpu, cpu):
                env.reset(seed=seed + 1, options={"mask": np.arange(n) % 3 == case % 3})
    assert ran >= 2, f"case {case}: only {ran} launches ran"
    g = gpu.state.clone_blocks()
    assert int(g["i32"][_abi.I32.SPARK_COUNT, :n].sum()) + int(g["i32"][_abi.I32.EPISODE, :n].sum()) > 0


@pytest.mark.parametrize("case", range(CASES))
def test_wire_material_forms_match_the_oracle(case):
    _fuzz(case)
