"""Per-environment draws of every randomisable physics parameter (`sparc_amd.core.env_params.NAMES`), shared by the CPU
oracle tests and the GPU fuzz.

Each of the 15 names is drawn independently per environment.  The ranges hold those of the uniform fuzz
(`_fuzz_case` in tests/test_gpu_parity.py) and put both sides of every edge of the model into one batch: ``zeta`` below
and above 1, ``sigmoid_steepness`` in {50, 500, 5000}, ``max_critical_density`` below ``base_critical_density`` for some
environments, ``hard_short_gap`` across the gaps the tests draw (0.5 to 30 um), the three clamps of the mechanics
(``max_speed``, ``max_acceleration``, ``max_jerk``) from values that bind at every step to values that never do, and
dielectric temperatures that are not float32-exact.  All limits stay positive (the physical domain)."""
from __future__ import annotations

import dataclasses

import numpy as np

from sparc_amd import (DielectricModuleParameters, IgnitionModuleParameters, MechanicsModuleParameters,
                       WireModuleParameters)
from sparc_amd.core import env_params as envp

CLS = {"ignition_params": IgnitionModuleParameters, "wire_params": WireModuleParameters,
       "dielectric_params": DielectricModuleParameters, "mechanics_params": MechanicsModuleParameters}


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def draw(rng: np.random.Generator, n: int) -> dict:
    """name -> float64 [n], every name drawn on its own."""
    u = lambda lo, hi: rng.uniform(lo, hi, n)  # noqa: E731
    out = {
        "base_critical_density": u(0.05, 0.4),
        "gap_coefficient": u(0.005, 0.03),
        "max_critical_density": u(0.02, 0.99),
        "hard_short_gap": u(0.3, 6.0),
        "sigmoid_steepness": rng.choice([50.0, 500.0, 5000.0], n),
        "spark_voltage_factor": u(0.2, 0.5),
        "debris_removal_efficiency": u(0.002, 0.05),
        "dielectric_temperature": u(285.0, 300.0),
        "plasma_efficiency": u(0.05, 0.3),
        "base_convection_coefficient": u(8000.0, 20000.0),
        "omega_n": u(150.0, 400.0),
        "zeta": u(0.2, 1.8),
        "max_acceleration": _log_uniform(rng, 1e3, 1e6, n),
        "max_jerk": _log_uniform(rng, 1e6, 1e11, n),
        "max_speed": _log_uniform(rng, 3.0, 4.5e4, n),
    }
    assert tuple(out) == envp.NAMES
    return out


def omega_26bit(x: np.ndarray) -> np.ndarray:
    """``omega_n`` values with at most 26 significant bits, as `uniform_param_sampler` draws them."""
    return (np.asarray(x, dtype=np.float64).view(np.int64) & ~((1 << 27) - 1)).view(np.float64)


def column(values: dict, e: int) -> dict:
    return {k: float(v[e]) for k, v in values.items()}


def uniform_kw(values: dict, base: dict | None = None) -> dict:
    """The dataclass keywords of an environment whose uniform parameters are `values` (name -> float), on top of the
    dataclasses in `base` (keyword -> instance) where given."""
    base = base or {}
    return {src: dataclasses.replace(base.get(src) or c(), **{n: values[n] for n, s in envp.SOURCES.items() if s == src})
            for src, c in CLS.items()}


def spread_ok(values: dict) -> None:
    """The draws did not collapse: every name takes several values, and each edge has both sides in the batch."""
    for name, v in values.items():
        assert len(np.unique(v)) >= 2, name
    z = values["zeta"]
    assert (z < 1).any() and (z > 1).any()
    assert (values["max_critical_density"] < values["base_critical_density"]).any()
    assert (values["max_critical_density"] > values["base_critical_density"]).any()
    t = values["dielectric_temperature"]
    assert (t.astype(np.float32).astype(np.float64) != t).any()
