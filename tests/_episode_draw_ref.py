"""The CPU definition of `wedm_draw_episode` (include/wedm_hip.h), written independently of
`sparc_amd.randomize`: one environment at a time, in Python floats and ints, with its Philox words from the oracle library
(`oracle.philox`) and its geometry rows from the stand-in of `wedm_derive_geometry` (`tests._geometry_ref`).

`draw_columns` works on a dict of NumPy blocks in place, so the same function serves an environment's blocks (host tests) and
raw guarded allocations (the kernel's memory contract).  `guarded_blocks` builds such allocations.
"""
from __future__ import annotations

import struct

import numpy as np

from oracle import oracle as orc
from sparc_amd import _abi
from sparc_amd.core.env_params import NAMES
from tests import _geometry_ref as gref

E = _abi.ENVP
SLOT_MATERIAL, SLOT_HEIGHT, SLOT_DIAMETER = 15, 16, 17
POISON = 0xA5
# the device row that holds a name's value itself
SAME_ROW = {"base_critical_density": E.BASE_CRITICAL_DENSITY, "gap_coefficient": E.GAP_COEFFICIENT,
            "max_critical_density": E.MAX_CRITICAL_DENSITY, "hard_short_gap": E.HARD_SHORT_GAP,
            "sigmoid_steepness": E.SIGMOID_STEEPNESS, "spark_voltage_factor": E.SPARK_VOLTAGE_FACTOR,
            "dielectric_temperature": E.DIELECTRIC_TEMPERATURE, "plasma_efficiency": E.PLASMA_EFFICIENCY,
            "base_convection_coefficient": E.BASE_CONVECTION, "omega_n": E.OMEGA_N, "max_acceleration": E.MAX_ACCELERATION,
            "max_speed": E.MAX_SPEED}


def word(seed: int, gid: int, k: int, slot: int) -> int:
    """The uint32 of slot ``slot`` for global environment ``gid`` at draw ``k``."""
    ctr = (k & 0xFFFFFFFF, 0, gid & 0xFFFFFFFF, 0x80000000 + (slot >> 2))
    return int(orc.philox(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[slot & 3])


def uniform(w: int, lo: float, hi: float, clear27: bool = False) -> float:
    u = (float(w) + 0.5) * 2.0 ** -32
    x = lo + (hi - lo) * u
    x = min(max(x, lo), hi)
    if clear27:
        (bits,) = struct.unpack("<q", struct.pack("<d", x))
        (x,) = struct.unpack("<d", struct.pack("<q", bits & ~((1 << 27) - 1)))
    return x


def choice(w: int, k: int) -> int:
    return (w * k) >> 32


def values(spec, seed: int, gid: int, k: int) -> dict:
    """What global environment ``gid`` draws at draw ``k``: name -> value, ``"wire_material"``, ``"workpiece_height"``,
    ``"wire_diameter_index"``.  ``spec``: ``{"params": {name: (lo, hi)}, "materials": K or None, "height": (lo, hi) or None,
    "diameters": K or None}``."""
    out = {}
    for name, (lo, hi) in spec.get("params", {}).items():
        out[name] = uniform(word(seed, gid, k, NAMES.index(name)), float(lo), float(hi), name == "omega_n")
    if spec.get("materials"):
        out["wire_material"] = choice(word(seed, gid, k, SLOT_MATERIAL), spec["materials"])
    if spec.get("height") is not None:
        out["workpiece_height"] = uniform(word(seed, gid, k, SLOT_HEIGHT), float(spec["height"][0]), float(spec["height"][1]))
    if spec.get("diameters"):
        out["wire_diameter_index"] = choice(word(seed, gid, k, SLOT_DIAMETER), spec["diameters"])
    return out


def draw_columns(b: dict, spec, seed: int, env_id_offset: int, num_envs: int, mask=None, consts=None, geom=None) -> int:
    """`wedm_draw_episode` on the NumPy blocks of ``b``, in place; returns the geometry status word.

    ``b``: ``count`` int32 [stride]; ``envp_src`` [15, stride], ``envp_rows`` [16, stride]; ``mat_index`` int64 [stride],
    ``wmat_table`` [M, 5, stride], ``wmat_rows`` [5, stride], ``wmat_geom_table`` [M, 8, stride]; ``geom_f64`` [8, stride],
    ``geom_i32`` [6, stride], ``height`` [stride], ``dia`` int32 [stride] -- those the spec needs.  ``consts``:
    ``base_flow_rate`` and ``dt_s``.  ``geom``: None (geometry rows are selected from the table) or, with dynamic geometry,
    ``{"wire", "combo", "n_diameters", "n_seg_max"}`` of `tests._geometry_ref.derive_columns`."""
    asked = np.ones(num_envs, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    params = spec.get("params", {})
    for e in np.flatnonzero(asked):
        e = int(e)
        k = int(b["count"][e])
        v = values(spec, seed, (env_id_offset + e) & 0xFFFFFFFF, k)
        if params:
            src, rows = b["envp_src"], b["envp_rows"]
            for name in params:
                src[NAMES.index(name), e] = v[name]
                if name in SAME_ROW:
                    rows[SAME_ROW[name], e] = v[name]
            get = lambda name: float(src[NAMES.index(name), e])  # noqa: E731  (drawn or stored)
            if "debris_removal_efficiency" in params:
                rows[E.DEBRIS_REMOVAL_PER_US, e] = get("debris_removal_efficiency") * consts["base_flow_rate"] * 1e-6
            if "omega_n" in params or "zeta" in params:
                rows[E.DAMPING_COEFF, e] = -2.0 * get("zeta") * get("omega_n")
            if "omega_n" in params:
                rows[E.STIFFNESS_COEFF, e] = -(get("omega_n") * get("omega_n"))
            if "max_jerk" in params:
                rows[E.MAX_JERK_DT, e] = get("max_jerk") * consts["dt_s"]
        if "wire_material" in v:
            m = v["wire_material"]
            b["mat_index"][e] = m
            b["wmat_rows"][:, e] = b["wmat_table"][m, :, e]
            if geom is None:
                b["geom_f64"][:, e] = b["wmat_geom_table"][m, :, e]
        if "workpiece_height" in v:
            b["height"][e] = v["workpiece_height"]
        if "wire_diameter_index" in v:
            b["dia"][e] = v["wire_diameter_index"]
        b["count"][e] = k + 1
    status = 0
    touches_geometry = bool(spec.get("materials")) or spec.get("height") is not None or bool(spec.get("diameters"))
    if geom is not None and touches_geometry and asked.any():
        n = num_envs
        safe = lambda a, fill: np.where(asked, a[:n], fill)  # noqa: E731  (unmasked columns may hold anything)
        mats = safe(b["mat_index"], 0) if "mat_index" in b else None
        status = gref.derive_columns(b["geom_f64"], b["geom_i32"], geom["wire"], geom["combo"], geom["n_diameters"],
                                     geom["n_seg_max"], safe(b["height"], 1.0), safe(b["dia"], 0), mats, asked)
    return status


# ------------------------------------------------------------------------------------------------ guarded raw allocations
SHAPES = {"count": (None, np.int32), "envp_src": (15, np.float64), "envp_rows": (_abi.ENVP_COUNT, np.float64),
          "mat_index": (None, np.int64), "wmat_rows": (_abi.WMAT_COUNT, np.float64), "geom_f64": (_abi.GEOM_F64_COUNT, np.float64),
          "geom_i32": (_abi.GEOM_I32_COUNT, np.int32), "height": (None, np.float64), "dia": (None, np.int32)}


def poisoned(shape, dtype) -> np.ndarray:
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, POISON, dtype=np.uint8).view(dtype).reshape(shape)


def is_poison(a: np.ndarray) -> bool:
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


def guarded_blocks(num_envs: int, stride: int, n_materials: int, n_diameters: int, mask, rng, heights=(1.0, 10.0)):
    """``(alloc, tables)``: every written block as an allocation ``[rows + 2, stride]`` of 0xA5 bytes (a guard row before and
    behind; `inner` gives the block itself), with plausible inputs in the MASKED columns of the blocks the call reads
    (source rows, stored material, height and diameter, counts) and poison everywhere else; and the read-only tables."""
    asked = np.ones(num_envs, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    cols = np.flatnonzero(asked)
    alloc = {name: poisoned(((rows or 1) + 2, stride), dtype) for name, (rows, dtype) in SHAPES.items()}
    b = inner(alloc)
    b["count"][cols] = rng.integers(0, 1000, cols.size)
    b["envp_src"][:, cols] = rng.uniform(0.5, 2.0, (15, cols.size))
    b["mat_index"][cols] = rng.integers(0, n_materials, cols.size)
    b["height"][cols] = rng.uniform(*heights, cols.size)
    b["dia"][cols] = rng.integers(0, n_diameters, cols.size)
    tables = {"wmat_table": rng.uniform(1.0, 2.0, (n_materials, _abi.WMAT_COUNT, stride)),
              "wmat_geom_table": rng.uniform(1.0, 2.0, (n_materials, _abi.GEOM_F64_COUNT, stride))}
    return alloc, tables


def inner(alloc: dict) -> dict:
    """Views of the blocks inside their guard rows (1-D for the per-environment arrays)."""
    return {name: (a[1] if SHAPES[name][0] is None else a[1:-1]) for name, a in alloc.items()}
