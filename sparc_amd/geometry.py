"""Per-episode workpiece height and wire diameter, derived on the device.

An environment built with ``dynamic_geometry={"max_workpiece_height": H, "wire_diameters": (d0, d1, ...)}`` keeps each
environment's height (float64) and diameter index (int32) as device tensors -- the source of truth -- and derives the 8 + 6
geometry rows the any-geometry kernels read from them with one launch of `wedm_derive_geometry` (include/wedm_hip.h), with the
bits `sparc_amd.core.derive.derive_geometry` writes on the host.  The wire block is sized for ``H``.

The derivation is split where the device can follow the host bit for bit.  What depends on the diameter and the material
only (``s_area`` is a C ``pow`` on the host) is derived once per (material, diameter) pair by `derive_geometry` itself into
the *combination table* (`combination_table`); what depends on the height is IEEE add, divide, floor-divide, one multiply and
integer min / max, which the kernel and `derive.geometry_rows` evaluate alike.

`WireEDMEnv.set_geometry`, `get_geometry`, the re-derivation in `set_wire_material` and the geometry part of `state_dict` are
thin callers of the functions below.  Without a backend ``derive_geometry`` (the CPU oracle backends of the tests) the rows
come from `derive.geometry_rows` on the host, under the same mask and with the same refusals; that path is what the kernel
is checked against.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .core import derive

STATUS_HEIGHT, STATUS_CAPACITY, STATUS_INDEX = _abi.GEOM_STATUS_HEIGHT, _abi.GEOM_STATUS_CAPACITY, _abi.GEOM_STATUS_INDEX


def check_spec(spec) -> Tuple[float, Tuple[float, ...]]:
    """``(max_workpiece_height, wire_diameters)`` of a ``dynamic_geometry=`` argument."""
    if not isinstance(spec, dict) or set(spec) != {"max_workpiece_height", "wire_diameters"}:
        raise ValueError('dynamic_geometry must be {"max_workpiece_height": H, "wire_diameters": (d0, d1, ...)}')
    H = float(spec["max_workpiece_height"])
    if not (math.isfinite(H) and H > 0):
        raise ValueError(f"dynamic_geometry: max_workpiece_height must be finite and positive, got {H}")
    dias = tuple(float(d) for d in np.asarray(spec["wire_diameters"], dtype=np.float64).reshape(-1))
    if not dias or any(not (math.isfinite(d) and d > 0) for d in dias) or len(set(dias)) != len(dias):
        raise ValueError(f"dynamic_geometry: wire_diameters must be distinct positive diameters, got {dias}")
    return H, dias


def host_constants(wire) -> Tuple[int, int]:
    """``(zone_start0, contact_bottom0)``: the two integers of the derivation that do not depend on the environment
    (wire.py:151 and wire.py:229-231, 239 before the clamps)."""
    seg = wire.segment_len
    return int(wire.buffer_len_bottom // seg), max(0, int((wire.buffer_len_bottom - wire.contact_offset_bottom) / seg))


def combination_table(materials: Sequence, diameters: Sequence[float], wire, material_params, height: float = 1.0) -> np.ndarray:
    """``float64[len(materials) * len(diameters), GEOMC_COUNT]``, row ``m * len(diameters) + d``: what `derive_geometry`
    derives from (material, diameter) alone, taken from `derive_geometry` itself, and ``math.pi * (diameter / 2)``."""
    G = _abi.GEOMC
    out = np.zeros((len(materials) * len(diameters), _abi.GEOMC_COUNT), dtype=np.float64)
    for m, mat in enumerate(materials):
        for k, d in enumerate(diameters):
            g = derive.derive_geometry(height, d, wire, mat, material_params)
            row = out[m * len(diameters) + k]
            row[G.K_COND], row[G.TUF], row[G.A_SURF], row[G.S_AREA] = g.k_cond, g.tuf, g.a_surf, g.s_area
            row[G.JOULE_GEOM], row[G.KERF_BASE] = g.joule_geom, g.kerf_base
            row[G.PI_R] = math.pi * (float(d) / 2.0)  # dielectric.py:62, the product's first two factors
    return out


class DynamicGeometry:
    """What a dynamic-geometry environment keeps: the capacity, the catalogue, the combination table and, as device tensors
    of the environment's stride, each environment's height and diameter index (padding columns repeat the last one)."""

    def __init__(self, env, max_height: float, diameters: Tuple[float, ...], materials: Sequence, height: np.ndarray,
                 dia_index: np.ndarray, stride: int):
        wire = env.wire_params
        self.max_height, self.diameters, self.materials = max_height, diameters, tuple(materials)
        self.n_seg_max = derive.derive_geometry(max_height, diameters[0], wire, materials[0], env.material_params).n_seg
        self.zone_start0, self.contact_bottom0 = host_constants(wire)
        self.combo_host = combination_table(materials, diameters, wire, env.material_params)
        dev = env.device
        self.combo = torch.from_numpy(self.combo_host).to(dev)
        self.diameter_values = torch.tensor(diameters, dtype=torch.float64).to(dev)
        n = height.shape[0]
        pad = lambda a: np.concatenate([a, np.repeat(a[-1:], stride - n)])  # noqa: E731
        self.height = torch.from_numpy(pad(np.asarray(height, dtype=np.float64))).to(dev)
        self.dia = torch.from_numpy(pad(np.asarray(dia_index, dtype=np.int32))).to(dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.keep = None  # inputs of the launch in flight
        self.desc = None  # built once the geometry blocks exist (`bind`)

    def bind(self, env) -> None:
        wire = env.wire_params
        self.desc = _abi.GeomDeriveDesc(
            segment_len=float(wire.segment_len), buffer_len_bottom=float(wire.buffer_len_bottom),
            buffer_len_top=float(wire.buffer_len_top), contact_offset_top=float(wire.contact_offset_top),
            zone_start0=self.zone_start0, contact_bottom0=self.contact_bottom0, num_envs=env.num_envs,
            n_seg_max=self.n_seg_max, stride=env._geom_f64.shape[1], combo=self.combo.data_ptr(),
            n_diameters=len(self.diameters), n_materials=len(self.materials), geom_f64=env._geom_f64.data_ptr(),
            geom_i32=env._geom_i32.data_ptr())

    def fingerprint(self) -> bytes:
        """What of the geometry determines the physics of a continuation: the capacity, the catalogue and the table -- not
        the current rows, which change with every episode (heights and indices are checkpointed themselves)."""
        return (np.asarray([self.max_height, *self.diameters], dtype=np.float64).tobytes()
                + np.asarray([self.n_seg_max, self.zone_start0, self.contact_bottom0], dtype=np.int64).tobytes()
                + self.combo_host.tobytes())


def initial_index(d: np.ndarray, diameters: Tuple[float, ...]) -> np.ndarray:
    """Index into the catalogue of every initial diameter (host values, checked)."""
    idx = np.full(d.shape, -1, dtype=np.int32)
    for k, v in enumerate(diameters):
        idx[d == v] = k
    if (idx < 0).any():
        raise ValueError(f"wire_diameter {float(d[idx < 0][0])} is not in dynamic_geometry's wire_diameters {diameters}")
    return idx


def refusal_bits(dyn: DynamicGeometry, wire, h: np.ndarray, di: np.ndarray, mi: Optional[np.ndarray]) -> np.ndarray:
    """The status bits `wedm_derive_geometry` would set for every environment (0: accepted), by the kernel's own
    expressions in NumPy float64 (the same operand order, a true division).  For the host path only: on the device the
    kernel alone decides (`derive_rows`) -- torch is not asked to repeat a float64 comparison at the capacity's edge, where
    its division by a scalar (a multiplication by the reciprocal on the GPU) lands on the other side."""
    with np.errstate(invalid="ignore", over="ignore"):
        bad_h = ~(h > 0.0) | np.isinf(h)
        cells = ((np.float64(wire.buffer_len_bottom) + h) + np.float64(wire.buffer_len_top)) / np.float64(wire.segment_len)
        over = ~bad_h & ~(cells < np.float64(dyn.n_seg_max) + 1.0)
    bad_i = (di < 0) | (di >= len(dyn.diameters))
    if mi is not None:
        bad_i = bad_i | (mi < 0) | (mi >= len(dyn.materials))
    return bad_h * STATUS_HEIGHT + over * STATUS_CAPACITY + bad_i * STATUS_INDEX


def _column(env, value, dtype, what: str) -> torch.Tensor:
    n = env.num_envs
    if torch.is_tensor(value):
        if dtype == torch.int32 and (value.is_floating_point() or value.dtype == torch.bool):
            raise ValueError(f"{what} must be integers, got {value.dtype}")
        t = value.detach().to(device=env.device).reshape(-1)
        if dtype == torch.int32 and t.dtype != torch.int32:  # what does not fit lands outside every catalogue
            t = t.clamp(-1, 2**31 - 1)
        t = t.to(dtype)
    else:
        a = np.asarray(value).reshape(-1)
        if dtype == torch.int32:
            if not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{what} must be integers, got {a.dtype}")
            a = np.where((a >= 0) & (a < 2**31), a, -1).astype(np.int32)
        else:
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    if t.numel() == 1:
        t = t.expand(n)
    if t.shape != (n,):
        raise ValueError(f"{what} must be a scalar or have one value per environment ({n})")
    return t


def _mask(env, mask) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    m = torch.as_tensor(mask, device=env.device).reshape(-1).to(torch.bool)
    if m.shape != (env.num_envs,):
        raise ValueError(f"mask must have one entry per environment ({env.num_envs})")
    return m


def derive_rows(env, h: torch.Tensor, di: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Writes the geometry rows of the masked environments from the candidate heights ``h`` (float64 [num_envs]) and diameter
    indices ``di`` (int32 [num_envs]) and the environment's current materials; refused candidates leave their column as it
    was and set their bit in the status word.  Returns the bool tensor of the environments whose rows were written.
    Nothing is read back on the native path.  `wedm_derive_geometry` has no per-environment "accepted" output (one status
    word for the call), and torch is not asked to repeat the kernel's float64 comparisons, so which environments the
    kernel accepted is read off the rows on the device: their N_SEG entries are set to 0 (no wire has 0 cells) before the
    launch; what is still 0 behind it was refused and gets its old value back.
    ASSUMPTION: the fill, the launch and the restore are enqueued back to back on torch's current stream of the
    environment's device, which is the stream every other consumer of the geometry rows (`wedm_step`, `wedm_reset`,
    `wedm_wire_profile`, `wedm_copy_columns`, torch reads) is enqueued on too, so none of them can run between the fill and
    the restore.  A caller that steps this environment from a second stream must order that stream behind this call (as
    it must for the new rows themselves)."""
    dyn, n = env._dyn, env.num_envs
    mi = env._wmat_index[:n].to(torch.int32) if env._wmat_rows is not None else None
    backend = env._backend
    if hasattr(backend, "derive_geometry"):
        h, di = h.contiguous(), di.contiguous()
        m8 = None if mask is None else mask.to(torch.uint8).contiguous()
        n_seg = env._geom_i32[_abi.GI32.N_SEG, :n]
        old = n_seg.clone()
        if mask is None:
            n_seg.zero_()
        else:
            n_seg.masked_fill_(mask, 0)
        backend.derive_geometry(dyn.desc, h.data_ptr(), di.data_ptr(), None if mi is None else mi.data_ptr(),
                                None if m8 is None else m8.data_ptr(), dyn.status.data_ptr())
        dyn.keep = (h, di, mi, m8)  # the launch is asynchronous: its inputs live until the next one replaces them
        refused = n_seg == 0
        n_seg.copy_(torch.where(refused, old, n_seg))
        return ~refused if mask is None else mask & ~refused
    # host path: `derive.geometry_rows` for the accepted environments, the status word as the kernel would leave it
    asked = np.ones(n, dtype=bool) if mask is None else mask.cpu().numpy()
    di_h = di.cpu().numpy()
    mi_h = None if mi is None else mi.cpu().numpy()
    bits = refusal_bits(dyn, env.wire_params, h.cpu().numpy(), di_h, mi_h)
    dyn.status.bitwise_or_(int(np.bitwise_or.reduce(bits[asked])) if asked.any() else 0)
    sel = asked & (bits == 0)
    ids = np.flatnonzero(sel)
    if ids.size:
        dd = np.asarray(dyn.diameters, dtype=np.float64)[di_h[ids]]
        mats = dyn.materials[0] if mi_h is None else [dyn.materials[int(k)] for k in mi_h[ids]]
        gf, gi, _ = derive.geometry_rows(h.cpu().numpy()[ids], dd, env.wire_params, mats, env.material_params, int(ids.size))
        ids_t = torch.from_numpy(ids).to(env.device)
        env._geom_f64[:, ids_t] = torch.from_numpy(gf).to(env.device)
        env._geom_i32[:, ids_t] = torch.from_numpy(gi).to(env.device)
    return torch.from_numpy(sel).to(env.device)


def set_geometry(env, workpiece_height=None, wire_diameter_index=None, mask=None, reset: bool = True) -> None:
    dyn, n = _dynamic(env), env.num_envs
    m = _mask(env, mask)
    cur_h, cur_d = dyn.height[:n], dyn.dia[:n]
    h = cur_h if workpiece_height is None else _column(env, workpiece_height, torch.float64, "workpiece_height")
    di = cur_d if wire_diameter_index is None else _column(env, wire_diameter_index, torch.int32, "wire_diameter_index")
    if m is not None:
        h, di = torch.where(m, h, cur_h), torch.where(m, di, cur_d)
    written = derive_rows(env, h, di, m)
    cur_h.copy_(torch.where(written, h, cur_h))
    cur_d.copy_(torch.where(written, di, cur_d))
    if reset:
        env.reset(options=None if m is None else {"mask": m})


def rederive(env, mask=None) -> None:
    """The rows of the masked environments again from the stored heights and indices (after a change of material, a load)."""
    dyn, n = _dynamic(env), env.num_envs
    derive_rows(env, dyn.height[:n], dyn.dia[:n], _mask(env, mask))


def get_geometry(env) -> Dict[str, torch.Tensor]:
    dyn, n = _dynamic(env), env.num_envs
    return {"workpiece_height": dyn.height[:n].clone(),
            "wire_diameter": dyn.diameter_values.index_select(0, dyn.dia[:n].to(torch.int64)),
            "n_segments": env._geom_i32[_abi.GI32.N_SEG, :n].clone()}


def _dynamic(env) -> DynamicGeometry:
    if getattr(env, "_dyn", None) is None:
        raise RuntimeError('construct the environment with dynamic_geometry={"max_workpiece_height": H, "wire_diameters": '
                           '(...)} to give environments a new workpiece height or wire diameter per episode')
    return env._dyn


def status_text(status: int) -> Optional[str]:
    """What `check_errors` says about a non-zero status word of `set_geometry`."""
    what = [text for bit, text in ((STATUS_HEIGHT, "a workpiece height that is NaN, infinite or not positive"),
                                   (STATUS_CAPACITY, "a workpiece height above max_workpiece_height (its wire would have more "
                                    "cells than the wire block holds)"),
                                   (STATUS_INDEX, "a wire-diameter (or material) index outside the catalogue"))
            if status & bit]
    if not what:
        return None
    return ("set_geometry: " + "; ".join(what) + " (those environments kept the geometry they had).  The values were not read "
            "back when the rows were derived; this check reports and clears the flag")


def state(env) -> Dict[str, Any]:
    dyn = getattr(env, "_dyn", None)
    if dyn is None:
        return {"dynamic_geometry": None}
    n = env.num_envs
    return {"dynamic_geometry": {"max_workpiece_height": dyn.max_height, "wire_diameters": list(dyn.diameters),
                                 "workpiece_height": dyn.height[:n].detach().cpu().clone(),
                                 "wire_diameter_index": dyn.dia[:n].detach().cpu().clone()}}


def check_state(env, sd: Dict[str, Any]) -> None:
    dyn, theirs = getattr(env, "_dyn", None), sd.get("dynamic_geometry")
    mine = None if dyn is None else (dyn.max_height, list(dyn.diameters))
    got = None if theirs is None else (float(theirs["max_workpiece_height"]), [float(d) for d in theirs["wire_diameters"]])
    if mine != got:
        raise ValueError(f"checkpoint was taken with dynamic geometry (max_workpiece_height, wire_diameters) = {got}, this "
                         f"environment has {mine}: the capacity or the catalogue differs")
    if dyn is not None:
        for key, dtype in (("workpiece_height", torch.float64), ("wire_diameter_index", torch.int32)):
            t = theirs[key]
            if tuple(t.shape) != (env.num_envs,) or t.dtype != dtype:
                raise ValueError(f"checkpoint block {key!r} has shape {tuple(t.shape)} and dtype {t.dtype}, expected "
                                 f"({env.num_envs},) {dtype}")


def load_state(env, sd: Dict[str, Any]) -> None:
    """The stored heights and indices, and the rows derived from them again.  With ``wire_material=`` the caller loads the
    material index next and `set_wire_material` derives the rows (with the loaded materials): nothing is launched here."""
    dyn = getattr(env, "_dyn", None)
    if dyn is None:
        return
    n, theirs = env.num_envs, sd["dynamic_geometry"]
    dyn.height[:n].copy_(theirs["workpiece_height"])
    dyn.dia[:n].copy_(theirs["wire_diameter_index"])
    dyn.height[n:].copy_(dyn.height[n - 1: n].expand(dyn.height.shape[0] - n))
    dyn.dia[n:].copy_(dyn.dia[n - 1: n].expand(dyn.dia.shape[0] - n))
    if env._wmat_rows is None:
        rederive(env)
