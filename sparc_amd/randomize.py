"""Seeded per-episode domain randomisation, drawn by one device kernel.

An `EpisodeSampler` gives every environment new physics parameters, a wire material, a workpiece height and a wire diameter
for each new episode, as a pure function of ``(seed, global environment id, draw number)``: the variate of *slot* ``s`` is
word ``s & 3`` of Philox4x32-10 on the counter ``{draw number, 0, global id, 0x80000000 + (s >> 2)}`` under the key
``{seed & 0xffffffff, seed >> 32}`` -- the generator of the step kernels on streams the physics never uses.  The contract,
complete enough to reproduce a draw from C, is at `wedm_draw_episode` in include/wedm_hip.h.  Batch size, rank, launch shape
and what ran before do not enter a draw, so a randomised run can be repeated, resumed from a checkpoint and compared
between one process and eight.

On the native backend a draw is one launch of `wedm_draw_episode`: the drawn values, every device row that depends on them
(`core.env_params.AFFECTS`, the material rows, the geometry rows of `wedm_derive_geometry`'s device code) and the draw
counts, under the mask, with no host read.  A backend without ``draw_episode`` (the CPU oracle backends of the tests) takes
the *host path* below: the same definition in NumPy, with `philox4x32_10` here and `derive.geometry_rows` for the geometry
rows.  The kernel is checked against that path bit for bit.
"""
from __future__ import annotations

import hashlib
import math
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _abi
from . import geometry as _geometry
from .core import env_params as envp

_M32 = np.uint64(0xFFFFFFFF)
_OMEGA_N = envp.INDEX["omega_n"]


def philox4x32_10(counter, key) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Philox4x32-10 of ``counter`` (four uint32 arrays or scalars, broadcast against each other) under ``key`` (two):
    the four output words as uint32 arrays -- `philox4` of the kernels (csrc/wedm_portable.h)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _M32 for c in counter))
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _uniform(w: np.ndarray, lo: float, hi: float, span: float, clear27: bool) -> np.ndarray:
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    x = np.float64(lo) + np.float64(span) * u
    x = np.minimum(np.maximum(x, np.float64(lo)), np.float64(hi))
    if clear27:  # 26 significant bits: x * x is exact and equals x ** 2
        x = (x.view(np.int64) & ~np.int64((1 << 27) - 1)).view(np.float64)
    return x


def _choice(w: np.ndarray, k: int) -> np.ndarray:
    return ((w.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int64)


def _bounds(what: str, pair) -> Tuple[float, float]:
    try:
        lo, hi = (float(v) for v in pair)
    except (TypeError, ValueError):
        raise ValueError(f"range of {what} must be a (low, high) pair, got {pair!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"range of {what} must be finite with low <= high, got ({lo}, {hi})")
    return lo, hi


def _count(what: str, value) -> Optional[int]:
    """``False`` -> not drawn (None); ``True`` -> the environment's number of values, known at `bind` (0); an int K -> K."""
    if value is False or value is None:
        return None
    if value is True:
        return 0
    k = int(value)
    if k < 1:
        raise ValueError(f"{what} must be True, False or a positive number of values, got {value!r}")
    return k


class EpisodeSampler:
    """``EpisodeSampler(seed, params={"name": (lo, hi), ...}, materials=False, height=None, diameters=False)``.

    ``params``: physics parameters of `core.env_params.NAMES`, each uniform in ``[lo, hi]``.  ``materials=True``: one of the
    environment's ``wire_materials``, uniformly.  ``height=(lo, hi)``: the workpiece height [mm], uniform.
    ``diameters=True``: one of ``dynamic_geometry``'s wire diameters, uniformly.  (``materials`` and ``diameters`` also take
    the number of values itself, for `expected` without an environment.)

    A sampler serves ONE environment (`bind`): it owns that environment's draw counts, an int32 device array."""

    def __init__(self, seed: int, params: Optional[Dict[str, Tuple[float, float]]] = None, materials=False,
                 height: Optional[Tuple[float, float]] = None, diameters=False):
        self.seed = int(seed) & (2 ** 64 - 1)
        params = dict(params or {})
        envp.check_names(params)
        self.params = {name: _bounds(repr(name), params[name]) for name in envp.NAMES if name in params}
        self.n_materials = _count("materials", materials)
        self.height = None if height is None else _bounds("height", height)
        if self.height is not None and not self.height[0] > 0.0:
            raise ValueError(f"height range must have 0 < low <= high, got {self.height}")
        self.n_diameters = _count("diameters", diameters)
        self._env = None
        self._count: Optional[torch.Tensor] = None  # int32 [stride] on the environment's device
        self._pending = None  # (fingerprint, counts) of a `load_state_dict` before `bind`
        self._diameter_values = None
        self._desc = None
        self._keep = None  # the mask of the launch in flight

    # ------------------------------------------------------------------------------------------ the spec
    @property
    def draws_geometry(self) -> bool:
        return self.height is not None or self.n_diameters is not None

    def _slots(self):
        """``[(slot, kind, k, lo, hi, span)]`` of the drawn slots."""
        out = [(envp.INDEX[name], _abi.DRAW_UNIFORM, 0, lo, hi, hi - lo) for name, (lo, hi) in self.params.items()]
        if self.n_materials is not None:
            out.append((_abi.DRAW_SLOT_MATERIAL, _abi.DRAW_CHOICE, self.n_materials, 0.0, 0.0, 0.0))
        if self.height is not None:
            out.append((_abi.DRAW_SLOT_HEIGHT, _abi.DRAW_UNIFORM, 0, *self.height, self.height[1] - self.height[0]))
        if self.n_diameters is not None:
            out.append((_abi.DRAW_SLOT_DIAMETER, _abi.DRAW_CHOICE, self.n_diameters, 0.0, 0.0, 0.0))
        return out

    def fingerprint(self) -> str:
        """sha256 over what is drawn and from which ranges (not the seed, not the counts)."""
        if 0 in (self.n_materials, self.n_diameters):
            raise RuntimeError("the number of materials / diameters is the environment's: bind(env) first, or give the number")
        h = hashlib.sha256()
        for slot, kind, k, lo, hi, _ in self._slots():
            h.update(np.asarray([slot, kind, k], dtype=np.int64).tobytes() + np.asarray([lo, hi], dtype=np.float64).tobytes())
        return h.hexdigest()

    # ------------------------------------------------------------------------------------------ the pure function
    def _variates(self, gid: np.ndarray, k: np.ndarray) -> Dict[int, np.ndarray]:
        """slot -> drawn values (float64 for uniform slots, int64 for choices) of global ids ``gid`` at draw numbers ``k``."""
        slots = self._slots()
        key = (self.seed & 0xFFFFFFFF, self.seed >> 32)
        words = {q: philox4x32_10((k, 0, gid, _abi.DRAW_STREAM0 + q), key) for q in sorted({s[0] >> 2 for s in slots})}
        out = {}
        for slot, kind, n, lo, hi, span in slots:
            w = words[slot >> 2][slot & 3]
            out[slot] = _choice(w, n) if kind == _abi.DRAW_CHOICE else _uniform(w, lo, hi, span, slot == _OMEGA_N)
        return out

    def expected(self, global_ids, draw_numbers) -> Dict[str, np.ndarray]:
        """What the environments of ``global_ids`` receive at their ``draw_numbers``-th draw (0-based; both broadcast): the
        drawn physics parameters by name, ``"wire_material"`` (index), ``"workpiece_height"``, ``"wire_diameter_index"`` and,
        once bound, ``"wire_diameter"``.  Evaluated on the host; no environment takes part."""
        if 0 in (self.n_materials, self.n_diameters):
            raise RuntimeError("the number of materials / diameters is the environment's: bind(env) first, or give the number")
        gid, k = np.broadcast_arrays(np.asarray(global_ids, dtype=np.int64), np.asarray(draw_numbers, dtype=np.int64))
        v = self._variates(gid.astype(np.uint64) & _M32, k.astype(np.uint64) & _M32)
        out = {name: v[envp.INDEX[name]] for name in self.params}
        if self.n_materials is not None:
            out["wire_material"] = v[_abi.DRAW_SLOT_MATERIAL]
        if self.height is not None:
            out["workpiece_height"] = v[_abi.DRAW_SLOT_HEIGHT]
        if self.n_diameters is not None:
            out["wire_diameter_index"] = v[_abi.DRAW_SLOT_DIAMETER]
            if self._diameter_values is not None:
                out["wire_diameter"] = self._diameter_values[v[_abi.DRAW_SLOT_DIAMETER]]
        return out

    # ------------------------------------------------------------------------------------------ the environment
    def bind(self, env) -> "EpisodeSampler":
        """Checks the spec against ``env`` and allocates its draw counts.  Done by the first `draw` otherwise."""
        if self._env is env:
            return self
        if self._env is not None:
            raise ValueError("this EpisodeSampler already serves another environment (it owns that one's draw counts); "
                             "make one sampler per environment")
        outside = [name for name in self.params if name not in env.env_param_names]
        if outside:
            raise ValueError(f"{outside} not randomised in this environment (env_params named {list(env.env_param_names)})")
        if self.n_materials is not None:
            if getattr(env, "_wmat_rows", None) is None:
                raise ValueError("materials=True needs an environment built with wire_material=[...] listing the materials")
            if self.n_materials not in (0, len(env.wire_materials)):
                raise ValueError(f"materials={self.n_materials}, the environment has {len(env.wire_materials)}")
        dyn = getattr(env, "_dyn", None)
        if self.draws_geometry and dyn is None:
            raise ValueError("height / diameters need an environment built with dynamic_geometry={...}")
        if self.n_diameters is not None and self.n_diameters not in (0, len(dyn.diameters)):
            raise ValueError(f"diameters={self.n_diameters}, the environment's dynamic_geometry has {len(dyn.diameters)}")
        if self.height is not None:
            hi = np.asarray([self.height[1]], dtype=np.float64)
            if int(_geometry.refusal_bits(dyn, env.wire_params, hi, np.zeros(1, dtype=np.int64), None)[0]):
                raise ValueError(f"height range {self.height} reaches above max_workpiece_height={dyn.max_height} (its wire "
                                 f"would have more cells than the wire block holds)")
        if self.n_materials is not None:
            self.n_materials = len(env.wire_materials)
        if self.n_diameters is not None:
            self.n_diameters = len(dyn.diameters)
            self._diameter_values = np.asarray(dyn.diameters, dtype=np.float64)
        stride = (env.num_envs + 63) // 64 * 64
        pending = None
        if self._pending is not None:  # a checkpoint loaded before the numbers of materials / diameters were known
            (theirs, pending), self._pending = self._pending, None
            if theirs != self.fingerprint():
                raise ValueError("the checkpoint's EpisodeSampler draws other names or from other ranges than this one")
            if pending is not None and tuple(pending.shape) != (env.num_envs,):
                raise ValueError(f"the checkpoint's draw counts are for {pending.shape[0]} environments, this sampler's "
                                 f"environment has {env.num_envs}")
        self._count = torch.zeros(stride, dtype=torch.int32, device=env.device)
        if pending is not None:
            self._count[: env.num_envs].copy_(pending)
        self._env = env
        if hasattr(env._backend, "draw_episode"):
            self._desc = self._descriptor(env)
        return self

    def _descriptor(self, env) -> "_abi.DrawDesc":
        d = _abi.DrawDesc(seed=self.seed, env_id_offset=env.env_id_offset & 0xFFFFFFFF, num_envs=env.num_envs,
                          stride=self._count.shape[0])
        for slot, kind, k, lo, hi, span in self._slots():
            d.slot[slot] = _abi.DrawSlot(kind=kind, k=k, lo=lo, hi=hi, span=span)
        consts = env._envp_consts()
        d.base_flow_rate, d.dt_s = consts["base_flow_rate"], consts["dt_s"]
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        d.envp_src, d.envp_rows = ptr(env._envp_src), ptr(env._envp_rows)
        if env._wmat_rows is not None:
            d.material_index, d.wmat_table, d.wmat_rows = ptr(env._wmat_index), ptr(env._wmat_table), ptr(env._wmat_rows)
            d.wmat_geom_table = ptr(env._wmat_geom_table)
        if env.per_env_geometry:
            d.geom_f64 = ptr(env._geom_f64)
        dyn = env._dyn
        if dyn is not None:
            d.dynamic, d.geom = 1, dyn.desc
            d.height, d.diameter_index, d.geom_status = ptr(dyn.height), ptr(dyn.dia), ptr(dyn.status)
        for t in (env._envp_src, env._wmat_rows, env._geom_f64 if env.per_env_geometry else None):
            if t is not None and t.shape[-1] != d.stride:
                raise RuntimeError(f"a per-environment block has stride {t.shape[-1]}, the draw counts {d.stride}")
        return d

    def draw(self, env, mask=None, reset: bool = True) -> None:
        """The next draw of the environments where ``mask`` (bool per environment; default: all) is set: their values, every
        row that depends on them and their draw counts, taking effect at the next launch.  With ``reset=True`` and a drawn
        geometry the masked environments are reset, as `WireEDMEnv.set_geometry` does (a new workpiece is a new episode);
        ``reset=False`` is for a caller whose next launch resets exactly those environments itself.  Nothing is read back."""
        self.bind(env)
        m = _geometry._mask(env, mask)
        if self._desc is not None:
            m8 = None if m is None else m.to(torch.uint8).contiguous()
            self._desc.seed = self.seed
            env._backend.draw_episode(self._desc, None if m8 is None else m8.data_ptr(), self._count.data_ptr())
            self._keep = m8  # the launch is asynchronous: its mask lives until the next one replaces it
        else:
            self._draw_on_host(env, m)
        if reset and self.draws_geometry:
            env.reset(options=None if m is None else {"mask": m})

    def _draw_on_host(self, env, m: Optional[torch.Tensor]) -> None:
        n = env.num_envs
        asked = np.ones(n, dtype=bool) if m is None else m.cpu().numpy()
        ids = np.flatnonzero(asked)
        if not ids.size:
            return
        at = torch.from_numpy(ids).to(env.device)
        count = self._count[:n]
        k = count.cpu().numpy()[ids]
        gid = (np.uint64(env.env_id_offset & 0xFFFFFFFF) + ids.astype(np.uint64)) & _M32
        v = self._variates(gid, k.astype(np.uint64) & _M32)

        def put(dst: torch.Tensor, values: np.ndarray) -> None:  # dst[..., ids] = values
            dst[..., at] = torch.from_numpy(np.ascontiguousarray(values)).to(device=env.device, dtype=dst.dtype)

        names = list(self.params)
        if names:
            for name in names:
                put(env._envp_src[envp.INDEX[name]], v[envp.INDEX[name]])
            src = {name: env._envp_src[envp.INDEX[name], :n].cpu().numpy()[ids] for name in envp.NAMES}
            consts = env._envp_consts()
            for r in sorted({r for name in names for r in envp.AFFECTS[name]}):
                if r == _abi.ENVP.STIFFNESS_COEFF:
                    row = -(src["omega_n"] * src["omega_n"])  # (exact: 26 significant bits)
                else:
                    row = envp.derive_row(r, src, consts)
                put(env._envp_rows[r], row)
        if self.n_materials is not None:
            mi = torch.from_numpy(v[_abi.DRAW_SLOT_MATERIAL]).to(env.device)
            env._wmat_index[at] = mi
            env._wmat_rows[:, at] = env._wmat_table[mi, :, at].t()
            if env._dyn is None:
                env._geom_f64[:, at] = env._wmat_geom_table[mi, :, at].t()
        dyn = env._dyn
        if dyn is not None and (self.n_materials is not None or self.draws_geometry):
            h, di = dyn.height[:n].clone(), dyn.dia[:n].clone()
            if self.height is not None:
                h[at] = torch.from_numpy(v[_abi.DRAW_SLOT_HEIGHT]).to(env.device)
            if self.n_diameters is not None:
                di[at] = torch.from_numpy(v[_abi.DRAW_SLOT_DIAMETER].astype(np.int32)).to(env.device)
            dyn.height[:n].copy_(h)
            dyn.dia[:n].copy_(di)
            _geometry.derive_rows(env, h, di, torch.from_numpy(asked).to(env.device))
        put(count, (k + 1).astype(np.int32))

    # ------------------------------------------------------------------------------------------ seed, counts, checkpoints
    def reseed(self, seed: int) -> None:
        """A new seed, and every environment back at draw 0."""
        self.seed = int(seed) & (2 ** 64 - 1)
        self._pending = None
        if self._count is not None:
            self._count.zero_()

    def draw_counts(self) -> torch.Tensor:
        """How many draws every environment has had (int32 [num_envs] device copy)."""
        if self._count is None:
            raise RuntimeError("bind(env) first: the draw counts live on the environment's device")
        return self._count[: self._env.num_envs].clone()

    def state_dict(self) -> Dict[str, Any]:
        return {"seed": self.seed, "fingerprint": self.fingerprint(),
                "draw_count": None if self._count is None else self.draw_counts().cpu()}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Seed and counts of `state_dict`.  A checkpoint of another spec is refused -- at once, or by `bind` when the
        numbers of materials / diameters are the environment's and no environment is bound yet."""
        deferred = self._count is None and 0 in (self.n_materials, self.n_diameters)
        if not deferred and sd["fingerprint"] != self.fingerprint():
            raise ValueError("the checkpoint's EpisodeSampler draws other names or from other ranges than this one")
        counts = sd["draw_count"]
        if counts is not None:
            counts = torch.as_tensor(counts).to(torch.int32).reshape(-1)
            if self._count is not None and counts.shape[0] != self._env.num_envs:
                raise ValueError(f"the checkpoint's draw counts are for {counts.shape[0]} environments, this sampler's "
                                 f"environment has {self._env.num_envs}")
        self.seed = int(sd["seed"]) & (2 ** 64 - 1)
        if self._count is None:
            self._pending = (sd["fingerprint"], counts)
        elif counts is None:
            self._count.zero_()
        else:
            self._count[: self._env.num_envs].copy_(counts)
