"""Per-environment physics parameters (domain randomisation): the set, the device rows, their derivation.

The user names a parameter by its field name in the module dataclasses (every name is unique across them).  The kernels
read one float64 row per device value (``enum wedm_envp_field``, include/wedm_hip.h); derived rows hold exactly what
`derive.build_params` writes into ``wedm_params`` for the same scalar inputs:

=============================  ===========  ====================================================================
user-facing                    dataclass    device row(s)
=============================  ===========  ====================================================================
base_critical_density,         Ignition     the value itself
gap_coefficient,
max_critical_density,
hard_short_gap,
sigmoid_steepness,
spark_voltage_factor
debris_removal_efficiency      Dielectric   debris_removal_per_us = eff * base_flow_rate * 1e-6
dielectric_temperature         Dielectric   the value (the float32 stencil rounds it to float32)
plasma_efficiency              Wire         the value
base_convection_coefficient    Wire         base_convection = the value
omega_n                        Mechanics    damping_coeff = -2.0 * zeta * omega_n, stiffness_coeff = -(omega_n ** 2),
                                            omega_n
zeta                           Mechanics    damping_coeff
max_acceleration, max_speed    Mechanics    the value
max_jerk                       Mechanics    max_jerk_dt = max_jerk * dt_s
=============================  ===========  ====================================================================

Left out on purpose: the ``random_short_*`` fields (``has_random_short`` is a wave-uniform switch of the kernels), the
crater and current tables, material properties and ``tcrit`` / ``tbreak`` (the served kernels' no-break proof relies on
them), and geometry (which has its own per-environment rows: ``workpiece_height`` / ``wire_diameter``).

``omega_n ** 2`` is C ``pow`` in Python, which differs from the correctly rounded ``x * x`` that torch and NumPy compute
for about one value in a thousand.  Host inputs (scalars, sequences, NumPy arrays, CPU tensors) are therefore derived
element by element in Python floats, exactly as `build_params` does.  Device tensors are derived on the device without a
host round trip, where the square is ``x * x``: that equals ``x ** 2`` whenever ``x`` has at most 26 significant bits
(the product is then exact, and so is C ``pow``), which `uniform_param_sampler` guarantees for its ``omega_n`` draws.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from .. import _abi

# user-facing name -> attribute of the environment holding the dataclass
SOURCES: Dict[str, str] = {
    "base_critical_density": "ignition_params",
    "gap_coefficient": "ignition_params",
    "max_critical_density": "ignition_params",
    "hard_short_gap": "ignition_params",
    "sigmoid_steepness": "ignition_params",
    "spark_voltage_factor": "ignition_params",
    "debris_removal_efficiency": "dielectric_params",
    "dielectric_temperature": "dielectric_params",
    "plasma_efficiency": "wire_params",
    "base_convection_coefficient": "wire_params",
    "omega_n": "mechanics_params",
    "zeta": "mechanics_params",
    "max_acceleration": "mechanics_params",
    "max_jerk": "mechanics_params",
    "max_speed": "mechanics_params",
}
NAMES: Tuple[str, ...] = tuple(SOURCES)
INDEX = {n: i for i, n in enumerate(NAMES)}

E = _abi.ENVP
# the value itself
_COPY = {
    "base_critical_density": E.BASE_CRITICAL_DENSITY, "gap_coefficient": E.GAP_COEFFICIENT,
    "max_critical_density": E.MAX_CRITICAL_DENSITY, "hard_short_gap": E.HARD_SHORT_GAP,
    "sigmoid_steepness": E.SIGMOID_STEEPNESS, "spark_voltage_factor": E.SPARK_VOLTAGE_FACTOR,
    "dielectric_temperature": E.DIELECTRIC_TEMPERATURE, "plasma_efficiency": E.PLASMA_EFFICIENCY,
    "base_convection_coefficient": E.BASE_CONVECTION, "omega_n": E.OMEGA_N, "max_acceleration": E.MAX_ACCELERATION,
    "max_speed": E.MAX_SPEED,
}
# device rows that depend on each user-facing name
AFFECTS: Dict[str, Tuple[int, ...]] = {n: (int(r),) for n, r in _COPY.items()}
AFFECTS["omega_n"] = (int(E.DAMPING_COEFF), int(E.STIFFNESS_COEFF), int(E.OMEGA_N))
AFFECTS["zeta"] = (int(E.DAMPING_COEFF),)
AFFECTS["max_jerk"] = (int(E.MAX_JERK_DT),)
AFFECTS["debris_removal_efficiency"] = (int(E.DEBRIS_REMOVAL_PER_US),)


def uniform_values(env) -> Dict[str, float]:
    """The dataclass value of every name, as the environment was built (Python floats)."""
    return {n: float(getattr(getattr(env, src), n)) for n, src in SOURCES.items()}


def derive_row(row: int, src, consts: Dict[str, float]):
    """Device row `row` from the user-facing values `src` (name -> float64 NumPy array or torch tensor, all names), in the
    reference's operand order.  `consts`: ``base_flow_rate`` and ``dt_s`` (uniform).  NumPy input: the element-wise
    Python-float result (``**`` is C pow); torch input: the same expressions on the tensor's device (square as x * x)."""
    if row == E.DEBRIS_REMOVAL_PER_US:
        return src["debris_removal_efficiency"] * consts["base_flow_rate"] * 1e-6
    if row == E.DAMPING_COEFF:
        return -2.0 * src["zeta"] * src["omega_n"]
    if row == E.STIFFNESS_COEFF:
        w = src["omega_n"]
        if torch.is_tensor(w):
            return -(w * w)
        return -np.fromiter((v ** 2 for v in w.tolist()), dtype=np.float64, count=w.size)
    if row == E.MAX_JERK_DT:
        return src["max_jerk"] * consts["dt_s"]
    for n, r in _COPY.items():
        if r == row:
            return src[n]
    raise ValueError(f"no row {row}")


def derive_rows(src, consts: Dict[str, float]):
    """All ``ENVP_COUNT`` device rows, stacked (same kind as the inputs)."""
    rows = [derive_row(r, src, consts) for r in range(_abi.ENVP_COUNT)]
    return torch.stack(rows) if torch.is_tensor(rows[0]) else np.stack(rows)


def check_names(names) -> None:
    unknown = sorted(set(names) - set(NAMES))
    if unknown:
        raise ValueError(f"unknown per-environment parameter(s) {unknown}; the randomisable ones are {list(NAMES)}")


def host_column(name: str, value, n: int) -> np.ndarray:
    """A host value (scalar, sequence, NumPy array, CPU tensor) as float64 [n]; wrong length or non-finite values raise."""
    if torch.is_tensor(value):
        value = value.detach().cpu().numpy()
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n, float(a))
    a = a.reshape(-1) if a.ndim == 1 else a
    if a.shape != (n,):
        raise ValueError(f"env_params[{name!r}] must be a scalar or have one value per environment ({n}), got shape "
                         f"{tuple(np.shape(value))}")
    if not np.isfinite(a).all():
        raise ValueError(f"env_params[{name!r}] holds non-finite values")
    return a
