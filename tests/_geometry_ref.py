"""The CPU stand-in of `wedm_derive_geometry` (include/wedm_hip.h): the split derivation in NumPy float64.

What depends on (material, diameter) comes from the combination table, built by `derive_geometry` itself
(`sparc_amd.geometry.combination_table`); what depends on the height is evaluated here element-wise with the kernel's
expressions -- IEEE add / divide / multiply, ``np.floor_divide`` (NumPy's float ``//`` is CPython's ``float_divmod``),
truncation and integer min / max.  `derive_columns` also mirrors the contract: the mask, the three refusals and their status
bits, and which columns are written.
"""
from __future__ import annotations

import numpy as np

from sparc_amd import _abi
from sparc_amd.core.material_db import WireMaterial, get_material_db
from sparc_amd.geometry import combination_table, host_constants  # noqa: F401  (re-exported for the tests)

BRASS = get_material_db().get_wire_material("brass")
COPPER = WireMaterial(name="copper", density=8960, specific_heat=385, thermal_conductivity=401,  # the f14 fixture's copper
                      electrical_resistivity=1.68e-08, temperature_coefficient=0.00393, melting_point=1358,
                      breaking_temperature=1600)

GF, GI, GC = _abi.GF64, _abi.GI32, _abi.GEOMC
INT_NAMES = ("n_seg", "zone_start", "az_start", "az_end", "contact_bottom", "contact_top")  # order of the int32 rows
F64_NAMES = ("workpiece_height", "kerf_base", "cavity_coeff", "k_cond", "tuf", "a_surf", "s_area", "joule_geom")


def height_part(h, wire):
    """The six integers and the zone end of heights ``h`` (float64 array; positive, finite): dict of int64 arrays."""
    h = np.asarray(h, dtype=np.float64)
    seg, bb = np.float64(wire.segment_len), np.float64(wire.buffer_len_bottom)
    bt, cot = np.float64(wire.buffer_len_top), np.float64(wire.contact_offset_top)
    zs0, cb0 = host_constants(wire)
    n = np.maximum(1, np.trunc(((bb + h) + bt) / seg).astype(np.int64))
    ze = np.minimum(zs0 + np.floor_divide(h, seg).astype(np.int64), n)
    zs = np.minimum(zs0, ze)
    ct = np.minimum(n - 1, np.trunc(((bb + h) + cot) / seg).astype(np.int64))
    ct = np.minimum(n - 1, np.maximum(ct, ze))
    cb = np.maximum(0, np.minimum(cb0, zs - 1))
    return {"n_seg": n, "zone_start": zs, "zone_end": ze, "az_start": np.minimum(zs, n - 1), "az_end": np.minimum(ze, n),
            "contact_bottom": cb, "contact_top": ct}


def refusal_bits(h, di, mi, wire, n_seg_max, n_diameters, n_materials):
    """Status bits per environment (0: accepted)."""
    h = np.asarray(h, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cells = ((np.float64(wire.buffer_len_bottom) + h) + np.float64(wire.buffer_len_top)) / np.float64(wire.segment_len)
        bad_h = ~(h > 0.0) | np.isinf(h)
        over = ~bad_h & ~(cells < np.float64(n_seg_max) + 1.0)
    bad_i = (di < 0) | (di >= n_diameters) | (mi < 0) | (mi >= n_materials)
    return bad_h * 1 + over * 2 + bad_i * 4


def derive_columns(gf, gi, wire, combo, n_diameters, n_seg_max, height, dia_idx, mat_idx=None, mask=None):
    """`wedm_derive_geometry` on NumPy blocks ``gf`` [8, stride] / ``gi`` [6, stride], in place, for the
    ``len(height)`` environments; returns the status word."""
    n = len(height)
    di = np.asarray(dia_idx, dtype=np.int64)
    mi = np.zeros(n, dtype=np.int64) if mat_idx is None else np.asarray(mat_idx, dtype=np.int64)
    asked = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    bits = refusal_bits(height, di, mi, wire, n_seg_max, n_diameters, combo.shape[0] // n_diameters)
    status = int(np.bitwise_or.reduce(bits[asked])) if asked.any() else 0
    e = np.flatnonzero(asked & (bits == 0))
    h = np.asarray(height, dtype=np.float64)[e]
    c = combo[mi[e] * n_diameters + di[e]]
    ints = height_part(h, wire)
    gf[GF.HEIGHT, e] = h
    gf[GF.CAVITY_COEFF, e] = c[:, GC.PI_R] * h
    for row, col in ((GF.KERF_BASE, GC.KERF_BASE), (GF.K_COND, GC.K_COND), (GF.TUF, GC.TUF), (GF.A_SURF, GC.A_SURF),
                     (GF.S_AREA, GC.S_AREA), (GF.JOULE_GEOM, GC.JOULE_GEOM)):
        gf[row, e] = c[:, col]
    for row, name in zip(GI, INT_NAMES):
        gi[row, e] = ints[name]
    return status


def boundary_heights(seg: float, k_max: int = 300) -> np.ndarray:
    """Every ``k * seg`` for 1 <= k < k_max, one ulp above it and half an ulp (one ulp of the next binade down) below it."""
    k = np.arange(1, k_max, dtype=np.float64) * np.float64(seg)
    return np.concatenate([k, np.nextafter(k, np.inf), np.nextafter(k, 0.0)])
