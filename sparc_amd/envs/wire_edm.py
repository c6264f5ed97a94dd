"""Batched ``WireEDMEnv`` — the reference's Gymnasium surface
(envs/wire_edm.py:16-201) with a leading batch dimension, advanced by one fused HIP
kernel on an MI355X.

Same constructor keywords, same ``reset(seed=, options=)`` / ``step(action)`` tuples,
same ``EnvironmentConfig`` and ``*ModuleParameters``; additionally ``num_envs`` and
``device``.  Every per-environment scalar of the reference becomes a length-N tensor
(``env.state.workpiece_position`` ...), ``terminated``/``truncated`` are ``bool[N]``,
``info`` carries the reference's five keys as tensors.

Documented deviations from the single-environment reference:
  * ``reset`` also resets module-private state (short timers, debris, caches,
    ``prev_accel``); the reference leaks it across episodes;
  * a terminated environment is frozen until it is reset;
  * a ``current_mode`` without crater data raises ``ValueError`` when the action is
    passed to ``step`` (the reference raises at the first fresh spark after the latch);
  * ``obs`` is a fixed float32 vector (the reference returns ``{}``), refreshed at
    control steps; ``reward`` is 0 as in the reference;
  * randomness is a counter-based Philox4x32-10 stream per environment, not NumPy's
    PCG64: same distributions, different variates for the same seed.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .. import _abi
from .. import geometry as _geometry
from .. import profile as _profile
from .. import snapshot as _snapshot
from ..core import derive
from ..core import env_params as envp
from ..core.env_config import EnvironmentConfig
from ..core.material_db import get_material_db
from ..core.state import BatchedEDMState
from ..core.tables import CRATER, MAX_MODE, MODE_CURRENT, VALID_CRATER_MODES
from ..modules.parameters import (
    DielectricModuleParameters,
    IgnitionModuleParameters,
    MaterialModuleParameters,
    MechanicsModuleParameters,
    WireModuleParameters,
)


class Box:
    """Minimal stand-in for ``gymnasium.spaces.Box`` (gymnasium is optional)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

    def sample(self, rng: Optional[np.random.Generator] = None):
        rng = rng or np.random.default_rng()
        if np.issubdtype(self.dtype, np.integer):
            return rng.integers(int(self.low), int(self.high) + 1, size=self.shape).astype(self.dtype)
        return rng.uniform(self.low, self.high, size=self.shape).astype(self.dtype)

    def __repr__(self):
        return f"Box({self.low}, {self.high}, {self.shape}, {self.dtype})"


class DictSpace(dict):
    """Minimal stand-in for ``gymnasium.spaces.Dict``."""

    def sample(self, rng: Optional[np.random.Generator] = None):
        return {k: v.sample(rng) for k, v in self.items()}


class StepInfo(dict):
    """``info`` of `step`: the reference's five keys (wire_edm.py:150-156) as tensors over the batch.  ``"time"`` is the
    exact 64-bit clock (`state.time`), composed from its two 32-bit rows when it is READ -- a per-microsecond loop that
    never looks at it pays nothing.  (`env.state.time_low32` is the zero-copy row itself -- the signed int32 bits of the
    clock modulo 2**32 -- for loops that want no op at all; the in-kernel trace records that row too.)"""

    __slots__ = ("_state",)

    def __init__(self, base, state):
        super().__init__(base)  # ("time" is a placeholder entry: membership and key order of the reference's dict)
        self._state = state

    def __getitem__(self, key):
        return self._state.time if key == "time" else dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self]

    def values(self):
        return [self[k] for k in self]

    def copy(self):
        return StepInfo({k: dict.__getitem__(self, k) for k in self}, self._state)

    # CPython copies a dict subclass's stored values directly (`dict(info)`, `{**info}`, `dict.update`) unless the class
    # overrides `__iter__`; it then goes through `keys()` and `__getitem__`, which composes the clock.
    def __iter__(self):
        return dict.__iter__(self)

    # `copy.copy`, `copy.deepcopy` and `pickle`: a plain dict with the clock materialised (no reference to the live state)
    def __reduce__(self):
        return dict, (dict(self.items()),)

    def __repr__(self):
        return repr(dict(self.items()))


class DeviceAction:
    """An action already laid out for the kernel: five contiguous length-N device
    tensors (float64 x4, int32).  Build it once with ``env.make_action`` and pass it
    to ``step`` to avoid per-step host->device conversion."""

    __slots__ = ("servo", "target_voltage", "on_time", "off_time", "current_mode", "ptrs")

    def __init__(self, servo, target_voltage, on_time, off_time, current_mode):
        self.servo, self.target_voltage, self.on_time, self.off_time = servo, target_voltage, on_time, off_time
        self.current_mode = current_mode
        self.ptrs = _abi.ActionPtrs(servo.data_ptr(), target_voltage.data_ptr(), on_time.data_ptr(),
                                    off_time.data_ptr(), current_mode.data_ptr())


class WireEDMEnv:
    """Main-cut Wire-EDM environment, N environments in lock-step (1 us base step,
    1 ms control step).  See the module docstring."""

    metadata = {"render_modes": ["human"], "render_fps": 300}

    def __init__(
        self,
        *,
        num_envs: int = 1,
        device: Any = None,
        render_mode: Optional[str] = None,
        mechanics_control_mode: str = "position",
        config: Optional[EnvironmentConfig] = None,
        ignition_params: Optional[IgnitionModuleParameters] = None,
        wire_params: Optional[WireModuleParameters] = None,
        material_params: Optional[MaterialModuleParameters] = None,
        dielectric_params: Optional[DielectricModuleParameters] = None,
        mechanics_params: Optional[MechanicsModuleParameters] = None,
        workpiece_height=None,
        wire_diameter=None,
        env_id_offset: int = 0,
        disable_ignition: bool = False,
        strict_actions: bool = True,
        autoreset: bool = False,
        reward: Optional[str] = None,
        reward_break_penalty: float = 10.0,
        stencil_dtype: str = "float32",
        crater_log_capacity: int = 0,
        reset_semantics: str = "full",
        freeze_terminated: bool = True,
        pulse_stats: bool = False,
        signal_stats: bool = False,
        env_params: Optional[Dict[str, Any]] = None,
        wire_material=None,
        wire_material_table=None,
        dynamic_geometry: Optional[Dict[str, Any]] = None,
        backend: Optional[Callable] = None,
    ):
        """Beyond the reference's keywords (wire_edm.py:22-34):

        ``autoreset``: next-step autoreset inside the launch — an environment found terminated when a
        step begins is reset by that kernel launch (as ``reset(options={"mask": done})`` would: next
        Philox episode, fresh module state) and then stepped; no host round trip.
        ``reward``: None = the reference's constant 0.0 (its `_calculate_reward` is a TODO,
        wire_edm.py:185-187); ``"progress"`` = micrometres the workpiece front advanced during the
        launch minus ``reward_break_penalty`` if the wire broke, written by the kernels (float32).
        ``stencil_dtype``: ``"float32"`` = the wire stencil exactly as the reference evaluates
        wire.py:58-123 without Numba (NumPy-2 scalar promotion: float32 op for op); ``"float64"`` =
        as Numba types the same lines (float64 expressions rounded at each float32 store).
        ``crater_log_capacity``: keep the last that many sampled crater volumes of every environment
        (`MaterialRemovalModule.crater_volumes_um3`, material.py:133) — see `get_crater_volumes`.
        ``reset_semantics``: ``"full"`` = a reset is a fresh environment, module-private state included (default);
        ``"reference"`` = exactly what the reference's ``reset()`` does (wire_edm.py:106-114): only ``EDMState`` is
        re-initialised, the module objects live on — ignition short timers and current cache, debris volume and
        the flow / density caches, ``prev_accel``, convection cache and coefficients, crater list and statistics
        carry over into the next episode (what every RL loop on the reference sees from its second episode on).
        ``freeze_terminated``: True = a terminated environment is frozen until it is reset (default); False = it
        keeps being stepped as the reference does when ``step()`` is called after ``terminated`` (wire_edm.py:116-157
        has no guard): after a wire break the wire module returns at once and the step returns before mechanics
        and clocks, after the cutting target everything goes on; ``terminated`` then repeats what the reference's
        ``step()`` returns.
        ``pulse_stats``: count, inside the kernels, the reference driver's "Sparks" and "Short pulses"
        (experiments/run_simulation.py:597-636) and the short-circuit steps of every control interval; the observation
        gains three columns (``spark_pulses``, ``short_pulses``, ``short_steps`` of the last completed interval: ``obs_dim``
        11) and `get_pulse_statistics` returns them.  Needs a backend with ``bind_pulse_stats`` (the HIP library).
        ``signal_stats``: sum, inside the kernels, what went into the gap over every control interval and keep its extrema:
        the current, the energy ``voltage * current`` and the gap ``workpiece_position - wire_position`` summed over the
        interval's physics steps, the smallest gap and the highest ``wire_max_temperature`` (include/wedm_hip.h, enum
        wedm_sig_field).  The observation gains the five columns `SIGNAL_OBS_NAMES` (raw float32 sums of the last completed
        interval, behind the pulse columns when both are on: ``obs_dim`` 13 or 16) and `get_signal_statistics` returns the
        float64 values and the interval's means.  Combines with every other keyword.  Needs a backend with
        ``bind_signal_stats`` (the HIP library).
        ``env_params``: domain randomisation -- a dict from physics-parameter names (the dataclass field names listed in
        `sparc_amd.core.env_params`: ignition thresholds, flushing efficiency, dielectric temperature, plasma heat share,
        convection, servo dynamics) to a scalar or one value per environment (sequence, NumPy array or tensor).  Names
        not given keep the uniform dataclass value.  The named set is fixed for the environment's life; the values can
        be changed between launches with `set_env_params` and read with `get_env_params`.  The random-short
        parameters, crater / current tables, material properties and geometry are not in the set (geometry and the wire
        material have their own per-environment keywords).  Needs a backend with ``bind_env_params`` (the HIP library).
        ``wire_material``: one wire material per environment -- a sequence of ``num_envs`` material names (looked up in
        `get_material_db()`) or `WireMaterial` objects.  The distinct materials, in order of first appearance, form
        ``env.wire_materials``, fixed for the environment's life; `set_wire_material` moves environments between them
        between launches (mid-episode too: the next launch steps the same wire temperatures with the new material), and
        `get_wire_material_index` reads the current choice.  ``config.wire_material`` stays the material of the uniform
        parameters, and ``env.wire_material`` (and ``env.wire.wire_material``) keep reporting it: the per-environment
        materials are ``env.wire_materials[env.get_wire_material_index()]``.  Implies per-environment geometry (the
        geometry rows carry the material's conductivity and heat capacity), even with uniform height and diameter: as for
        any per-environment geometry, ``zone_mean_temperature()`` and the ``wire_average_temperature`` signal then come from
        `wire_profile` (each environment's own zone).  Combines with ``workpiece_height`` / ``wire_diameter``, ``env_params``, ``pulse_stats``,
        ``stencil_dtype``, ``autoreset`` and ``reward``.  Needs a backend with ``bind_wire_material`` (the HIP library).
        ``wire_material_table``: the materials of ``env.wire_materials`` in a fixed order (names or `WireMaterial`
        objects), so that indices mean the same materials in several environments (the shards of one batch); every
        entry of ``wire_material`` must be one of them.
        ``dynamic_geometry``: ``{"max_workpiece_height": H, "wire_diameters": (d0, d1, ...)}`` -- a new workpiece height and
        wire diameter per episode.  Implies per-environment geometry; the wire block is sized for ``H``.  ``workpiece_height``
        / ``wire_diameter`` give the initial values (heights of at most ``H``, diameters from the list; default:
        ``config``'s pair, whose diameter must be in the list).  `set_geometry` gives environments new values between
        launches, derived on the device (`sparc_amd.geometry`), `get_geometry` reads them.  Heights
        and diameter indices are then state: `snapshot` / `restore` / `fork` carry them and the geometry rows, and
        `state_dict` saves them.  Combines with ``wire_material`` (whose `set_wire_material` re-derives the rows), ``env_params``
        and the statistics keywords; runs on the any-geometry kernels (1, 2, 10, 11)."""
        self.render_mode = render_mode
        if mechanics_control_mode not in ["position", "velocity"]:
            raise ValueError(f"mechanics_control_mode must be 'position' or 'velocity', got {mechanics_control_mode}")
        self.mechanics_control_mode = mechanics_control_mode
        if int(num_envs) <= 0:
            raise ValueError("num_envs must be positive")
        self.num_envs = int(num_envs)

        self.config = config or EnvironmentConfig()
        self.config.validate()
        self.dt = self.config.dt
        self.servo_interval = self.config.servo_interval

        self.ignition_params = ignition_params or IgnitionModuleParameters()
        self.wire_params = wire_params or WireModuleParameters()
        self.material_params = material_params or MaterialModuleParameters()
        self.dielectric_params = dielectric_params or DielectricModuleParameters()
        self.mechanics_params = mechanics_params or MechanicsModuleParameters()
        self.wire_material = get_material_db().get_wire_material(self.config.wire_material)

        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.np_random = np.random.default_rng()
        self.strict_actions = bool(strict_actions)
        self.env_id_offset = int(env_id_offset)
        self.autoreset = bool(autoreset)
        if reward not in (None, "progress"):
            raise ValueError("reward must be None (the reference's constant 0.0) or 'progress'")
        self.reward_kind = reward
        if reset_semantics not in ("full", "reference"):
            raise ValueError("reset_semantics must be 'full' or 'reference'")
        self.reset_semantics, self.freeze_terminated = reset_semantics, bool(freeze_terminated)
        if stencil_dtype not in ("float32", "float64"):
            raise ValueError("stencil_dtype must be 'float32' or 'float64'")
        self.stencil_dtype = stencil_dtype
        self.pulse_stats = bool(pulse_stats)
        if backend is not None and self.pulse_stats and not hasattr(backend, "bind_pulse_stats"):
            raise ValueError(f"pulse_stats=True needs a backend that counts pulses inside its step (bind_pulse_stats); "
                             f"{getattr(backend, '__name__', backend)!r} has none")
        self.signal_stats = bool(signal_stats)
        if backend is not None and self.signal_stats and not hasattr(backend, "bind_signal_stats"):
            raise ValueError(f"signal_stats=True needs a backend that tallies the interval's signals inside its step "
                             f"(bind_signal_stats); {getattr(backend, '__name__', backend)!r} has none")
        self.obs_names = _abi.OBS_NAMES + (_abi.PULSE_OBS_NAMES if self.pulse_stats else ()) + \
            (_abi.SIGNAL_OBS_NAMES if self.signal_stats else ())
        self.obs_dim = len(self.obs_names)
        if env_params is not None:
            if backend is not None and not hasattr(backend, "bind_env_params"):
                raise ValueError(f"env_params needs a backend that reads per-environment physics rows (bind_env_params); "
                                 f"{getattr(backend, '__name__', backend)!r} has none")
            env_params = dict(env_params)
            envp.check_names(env_params)
        if wire_material is not None:
            if backend is not None and not hasattr(backend, "bind_wire_material"):
                raise ValueError(f"wire_material needs a backend that reads per-environment wire-material rows "
                                 f"(bind_wire_material); {getattr(backend, '__name__', backend)!r} has none")
            self.wire_materials, mat_index = _material_table(wire_material, self.num_envs, wire_material_table)
        elif wire_material_table is not None:
            raise ValueError("wire_material_table needs wire_material=[...]")
        else:
            self.wire_materials, mat_index = (), None
        self._wmat_rows = None  # float64 [WMAT_COUNT, stride] device rows of the current materials (wire_material=)

        # ---- geometry: uniform (reference behaviour) or one (h, d) pair per environment
        stride = (self.num_envs + 63) // 64 * 64
        self._dyn = None  # `sparc_amd.geometry.DynamicGeometry` of an environment built with dynamic_geometry=
        dyn_spec = None if dynamic_geometry is None else _geometry.check_spec(dynamic_geometry)
        self.per_env_geometry = workpiece_height is not None or wire_diameter is not None or mat_index is not None or \
            dyn_spec is not None
        self._geom_hd = None  # float64 [2, num_envs]: each slot's (height, diameter), where they are not all the same
        if self.per_env_geometry:
            h = np.broadcast_to(np.asarray(self.config.workpiece_height if workpiece_height is None
                                           else _to_numpy(workpiece_height), dtype=np.float64), (self.num_envs,))
            d = np.broadcast_to(np.asarray(self.config.wire_diameter if wire_diameter is None
                                           else _to_numpy(wire_diameter), dtype=np.float64), (self.num_envs,))
            mats = self.wire_material
            if dyn_spec is not None:
                if not (np.isfinite(h).all() and (h > 0).all() and (h <= dyn_spec[0]).all()):
                    raise ValueError(f"workpiece_height must lie in (0, max_workpiece_height={dyn_spec[0]}] with "
                                     f"dynamic_geometry, got {float(h[~((h > 0) & (h <= dyn_spec[0]))][0])}")
                self._dyn = _geometry.DynamicGeometry(self, dyn_spec[0], dyn_spec[1], self.wire_materials or (self.wire_material,),
                                                      h, _geometry.initial_index(d, dyn_spec[1]), stride)
                if mat_index is not None:  # (no per-material row table at a fixed height: the rows are derived)
                    mats = [self.wire_materials[k] for k in mat_index]
            gf, gi, n_seg_max = derive.geometry_rows(h, d, self.wire_params, mats, self.material_params, stride)
            self.geometry = None
            self._geom_f64 = torch.from_numpy(gf).to(self.device)
            self._geom_i32 = torch.from_numpy(gi).to(self.device)
            self.n_segments = n_seg_max
            if self._dyn is not None:
                self.n_segments = self._dyn.n_seg_max  # the capacity: n_seg is monotone in the height
                self._dyn.bind(self)
            elif (h != h[0]).any() or (d != d[0]).any():  # slots differ: `fork` / `restore` hold copies to equal pairs
                self._geom_hd = np.stack([h, d])
            if mat_index is not None:
                self._init_wire_material(h, d, mat_index, stride)
        else:
            self.geometry = derive.derive_geometry(self.config.workpiece_height, self.config.wire_diameter,
                                                   self.wire_params, self.wire_material, self.material_params)
            self.n_segments = self.geometry.n_seg
        self.params = derive.build_params(
            self.config, mechanics_control_mode, self.ignition_params, self.wire_params, self.material_params,
            self.dielectric_params, self.mechanics_params, self.wire_material, geometry=self.geometry,
            env_id_offset=self.env_id_offset, obs_dim=self.obs_dim, disable_ignition=disable_ignition,
            autoreset=self.autoreset, reward_mode=1 if reward == "progress" else 0,
            reward_break_penalty=reward_break_penalty, stencil_mode=1 if stencil_dtype == "float64" else 0,
            reset_semantics=1 if reset_semantics == "reference" else 0, keep_stepping_terminated=not freeze_terminated)

        # ---- state (caller-owned memory) + backend
        self.state = BatchedEDMState(self.num_envs, self.n_segments, self.obs_dim, self.device,
                                     crater_log_capacity=int(crater_log_capacity), pulse_stats=self.pulse_stats,
                                     signal_stats=self.signal_stats)
        from ..utils.logger import dielectric_flow_rate

        base_flow = float(self.dielectric_params.base_flow_rate)
        self.state.derived["dielectric_flow_rate"] = lambda: dielectric_flow_rate(self.state.flow_rate, base_flow)
        self.state.derived["wire_average_temperature"] = self.zone_mean_temperature
        if backend is None:
            from .._lib import HipBackend

            backend = HipBackend
        self._backend = backend(self.params, self.num_envs, self.n_segments, self.device)
        self._backend.bind_state(self.state.pointers(with_obs=True))
        if self.per_env_geometry:
            self._backend.bind_geometry(_abi.GeomPtrs(self._geom_f64.data_ptr(), self._geom_i32.data_ptr()))
        if self.pulse_stats:
            self._backend.bind_pulse_stats(self.state.pulse.data_ptr())
        if self.signal_stats:
            self._backend.bind_signal_stats(self.state.signal.data_ptr())
        # ---- per-environment physics parameters (include/wedm_hip.h, enum wedm_envp_field), optional
        self.env_param_names: Tuple[str, ...] = ()
        self._envp_src = self._envp_rows = None  # float64 [len(envp.NAMES), stride] user-facing / [ENVP_COUNT, stride] device
        if env_params is not None:
            self._init_env_params(env_params, stride)
            self._backend.bind_env_params(self._envp_rows.data_ptr())
        if mat_index is not None:
            self._backend.bind_wire_material(self._wmat_rows.data_ptr())

        # what remains of the reference's module objects: parameters + read-only helpers
        from ..modules.views import DielectricView, IgnitionView, MaterialView, MechanicsView, WireView

        self.ignition = IgnitionView(self)
        self.wire = WireView(self)
        self.material = MaterialView(self)
        self.dielectric = DielectricView(self)
        self.mechanics = MechanicsView(self)
        self.modules = {"ignition": self.ignition, "material": self.material, "dielectric": self.dielectric,
                        "wire": self.wire, "mechanics": self.mechanics}

        # ---- spaces (wire_edm.py:84-101); obs is this build's fixed vector
        self.action_space = DictSpace({
            "servo": Box(-1.0, 1.0, (1,), np.float32),
            "generator_control": DictSpace({
                "target_voltage": Box(0.0, 200.0, (1,), np.float32),
                "current_mode": Box(1, 19, (1,), np.int32),
                "ON_time": Box(0.0, 5.0, (1,), np.float32),
                "OFF_time": Box(0.0, 100.0, (1,), np.float32),
            }),
        })
        self.observation_space = Box(-np.inf, np.inf, (self.obs_dim,), np.float32)
        self.single_action_space = self.action_space
        self.single_observation_space = self.observation_space

        self._reward = self.state.reward[0, : self.num_envs]  # zeros unless reward="progress" (written by the kernels)
        self._truncated = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        self._mask_buf = None
        # current modes with crater data (material.py:108-113) as a device-side lookup table: index mode, clamped to [0, 20]
        self._valid_modes_dev = torch.tensor([m in VALID_CRATER_MODES for m in range(MAX_MODE + 2)], dtype=torch.bool).to(self.device)
        self._step_out = None
        self._trace = None
        # status word of `snapshot` / `restore` / `fork` with device-resident indices (sparc_amd.snapshot; `check_errors`)
        self._copy_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        # `wire_profile` (sparc_amd.profile): its status word for device-resident indices, its output blocks by (bins, count)
        self._profile_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._profile_out: Dict[Tuple[int, int], torch.Tensor] = {}
        self._profile_keep = None
        self._seed = int.from_bytes(os.urandom(8), "little")
        self.steps_since_reset = 0  # host-side count of physics steps since the last reset of ALL environments
        self._backend.reset(None, self._seed, True, fresh=True)  # fresh module objects, whatever `reset_semantics`

    # ------------------------------------------------------------------ Gym API
    def reset(self, *, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        """``WireEDMEnv.reset`` (wire_edm.py:106-114).  ``options={"mask": bool[N]}``
        resets only the selected environments."""
        mask_ptr = None
        if options and options.get("mask") is not None:
            mask = torch.as_tensor(options["mask"]).to(self.device).reshape(-1).to(torch.uint8).contiguous()
            if mask.numel() != self.num_envs:
                raise ValueError("options['mask'] must have one entry per environment")
            self._mask_buf = mask  # keep alive until the launch has consumed it
            mask_ptr = mask.data_ptr()
        if seed is not None:
            self._seed = int(seed)
            self.np_random = np.random.default_rng(seed)
            self._backend.reset(mask_ptr, self._seed, True)
        else:
            self._backend.reset(mask_ptr, self._seed, False)
        if mask_ptr is None:
            self.steps_since_reset = 0
        return self._get_obs(), {}

    def step(self, action):
        """One 1-us physics step for every environment (wire_edm.py:116-157)."""
        return self.step_many(action, 1)

    def step_many(self, action, n_substeps: int):
        """``n_substeps`` consecutive ``step(action)`` calls in ONE fused kernel launch."""
        act = self._prepare_action(action)
        self._last_action = act  # keep the tensors alive while the launch is in flight
        n_substeps = int(n_substeps)
        # (`state.time` is 64-bit: the kernels carry its low word and bump the high word once per launch, so a single
        # launch may not advance an environment by 2**31 us or more; nothing limits the number of launches)
        if n_substeps * self.dt >= 2**31:
            raise ValueError(f"one launch may advance an environment by less than 2**31 us (asked: {n_substeps} x {self.dt} us)")
        self._backend.step(n_substeps, act.ptrs)
        self.steps_since_reset += n_substeps
        # obs / done / info are views of caller-owned memory the kernel has just (asynchronously)
        # updated: built once, handed out every step (`info` is a fresh dict of the same tensors)
        out = self._step_out
        if out is None:
            st = self.state
            out = self._step_out = (self._get_obs(), st.done, {
                "wire_broken": st.is_wire_broken,
                "target_reached": st.is_target_distance_reached,
                "spark_state": st.spark_state,
                "time": None,  # the exact int64 clock, composed when it is read (StepInfo)
                "control_step": st.control_step,
            })
        return out[0], self._reward, out[1], self._truncated, StepInfo(out[2], self.state)

    def step_control(self, action):
        """One control interval (``servo_interval`` physics steps, default 1000)."""
        return self.step_many(action, -(-self.servo_interval // self.dt))  # ceil: the latch tests `time_since_servo >= servo_interval`

    def close(self) -> None:
        self._backend.close()

    # ------------------------------------------------------------------ helpers
    def make_action(self, servo=0.0, target_voltage=80.0, current_mode=5, ON_time=3.0, OFF_time=80.0) -> DeviceAction:
        return self._prepare_action({
            "servo": servo,
            "generator_control": {"target_voltage": target_voltage, "current_mode": current_mode,
                                  "ON_time": ON_time, "OFF_time": OFF_time},
        })

    def _leaf(self, value, dtype) -> torch.Tensor:
        if torch.is_tensor(value):
            t = value.to(device=self.device, dtype=dtype).reshape(-1)
        else:
            arr = np.asarray(value)
            t = torch.from_numpy(np.ascontiguousarray(arr.reshape(-1))).to(device=self.device, dtype=dtype)
        if t.numel() == 1:
            t = t.expand(self.num_envs)
        elif t.numel() != self.num_envs:
            raise ValueError(f"action leaf has {t.numel()} values, expected 1 or num_envs={self.num_envs}")
        return t.contiguous()

    def _prepare_action(self, action) -> DeviceAction:
        if isinstance(action, DeviceAction):
            # the kernel reads num_envs elements through raw pointers: never let a foreign action through
            if action.servo.device != self.device or action.servo.numel() != self.num_envs:
                raise ValueError("DeviceAction belongs to another environment (device or num_envs differ); "
                                 "build it with this environment's make_action()")
            return action
        gc = action["generator_control"]
        mode = gc["current_mode"]
        if self.strict_actions:
            self._validate_modes(mode)
        return DeviceAction(
            self._leaf(action["servo"], torch.float64),
            self._leaf(gc["target_voltage"], torch.float64),
            self._leaf(gc["ON_time"], torch.float64),
            self._leaf(gc["OFF_time"], torch.float64),
            self._leaf(mode, torch.int32),
        )

    def _validate_modes(self, mode) -> None:
        """Mirror of material.py:108-113: modes without crater data are an error.

        Host-side values (Python numbers, NumPy arrays, CPU tensors) are checked here and raise at once.  A tensor that
        already lives on the device is checked ON the device and never read back: a policy that emits fresh device
        tensors every control step must not block on the previous launch (a `.cpu()` here waited for the 4-6 ms
        launch still in flight).  An invalid entry sets the environment's sticky ERROR flag -- the row the kernels
        set at the first fresh spark with such a mode -- and `check_errors()` raises for it (deferred raise)."""
        if torch.is_tensor(mode) and mode.device.type != "cpu":
            m = mode.to(self.device).reshape(-1).to(torch.int64)
            bad_dev = ~self._valid_modes_dev[torch.clamp(m, 0, MAX_MODE + 1)]  # (table built at construction: no upload here)
            if bad_dev.numel() == 1:
                bad_dev = bad_dev.expand(self.num_envs)
            elif bad_dev.numel() != self.num_envs:
                raise ValueError(f"action leaf has {bad_dev.numel()} values, expected 1 or num_envs={self.num_envs}")
            self.state.error.logical_or_(bad_dev)  # stream-ordered before the launch that latches the action
            return
        vals = mode.detach().numpy() if torch.is_tensor(mode) else np.asarray(mode)
        bad = sorted({int(v) for v in np.unique(vals.reshape(-1)) if int(v) not in VALID_CRATER_MODES})
        if bad:
            raise ValueError(
                f"Current mode I{bad[0]} is not available in crater data. "
                f"Available modes: {[f'I{m}' for m in VALID_CRATER_MODES]}"
            )

    def _get_obs(self) -> torch.Tensor:
        """``float32[num_envs, obs_dim]``: gap, wire_velocity, voltage, current, spark_state,
        debris_density, flow_rate, max wire temperature — as of each environment's last
        control step (the reference's ``_get_obs`` is a TODO, wire_edm.py:181-183) — and with
        ``pulse_stats`` the interval's spark pulses, short pulses and short-circuit steps (``obs_names``)."""
        return self.state.obs[:, : self.num_envs].t()

    def check_errors(self) -> None:
        """Synchronising check of the sticky per-environment error flag."""
        if bool(self.state.error.any().item()):
            idx = int(torch.nonzero(self.state.error)[0].item())
            raise ValueError(f"environment {idx}: a current mode that has no crater data was latched / passed in a device "
                             f"tensor (material.py:108-113 raises at the first fresh spark with it). "
                             f"Available modes: {[f'I{m}' for m in VALID_CRATER_MODES]}")
        status = int(self._copy_status.item())
        if status:
            self._copy_status.zero_()
            what = [text for bit, text in ((_snapshot.STATUS_RANGE, "an environment or snapshot-column index out of range (that "
                                            "pair was skipped)"),
                                           (_snapshot.STATUS_OVERLAP, "a destination named twice, or a source among the "
                                            "destinations (those environments hold one of the states copied into them)"))
                    if status & bit]
            raise ValueError("snapshot / restore / fork with indices in a device tensor: " + "; ".join(what)
                             + ".  The indices were not read back when the copy was launched; this check reports and clears "
                               "the flag")
        status = int(self._profile_status.item())
        if status:
            self._profile_status.zero_()
            raise ValueError(_profile.status_text(status))
        if self._dyn is not None:
            status = int(self._dyn.status.item())
            if status:
                self._dyn.status.zero_()
                raise ValueError(_geometry.status_text(status))

    def set_kernel(self, variant: int, lanes: int = 0) -> None:
        """0 = auto, 1 = global-memory stencil, 2 = LDS predicated, 3 = LDS fused, 4 = LDS
        fused with packed float32 math, 5 = global-memory stencil split over four waves, 6 =
        stream kernel (5 / 6: single microseconds; auto picks between them by shape), 7 = register
        kernel (one environment per lane, its whole wire in registers: wires of at most 128 segments,
        uniform geometry), 8 = wide register kernel (4 / 8 / 16 lanes per environment with 32 cells each in
        registers: wires of 9 to 512 segments, uniform geometry; auto picks it for fused launches of small
        batches), 9 = served kernel (kernel 4's walk with the float64 scalar physics of a block's environments on a wave
        of its own, one microsecond ahead of the walking waves: 4 or 8 lanes per environment, uniform geometry);
        10 = kernel 2's cell-by-cell form by name (kernel 2 is its packed form wherever the stencil is float32), 11 = the served
        form of kernel 2, 12 = the served form of kernel 7; ``lanes`` lanes per environment for 2/3/4/6/8/9/10/11 (0 = auto).
        All variants are bit-identical.  With ``stencil_dtype="float64"`` kernels 1, 2 / 10, 3, 6 (single microseconds without a
        trace sample), 7 and 8 accept the launch (the others raise ``WEDM_ERR_UNSUPPORTED``)."""
        self._backend.set_kernel(variant)
        if hasattr(self._backend, "set_lanes"):
            self._backend.set_lanes(lanes)

    def bind_trace(self, signals, *, every: int = 1, capacity: int = 1000, envs=None, wire_temperature: bool = False):
        """Record `signals` (EDMState attribute names, plus ``"wire_temperature"``) of the
        environments ``envs=(first, count)`` (default: all) every ``every`` microseconds INSIDE
        the step kernels, into a ring of ``capacity`` samples — what the reference does with
        `SimulationLogger.collect` after each 1-us step (utils/logger.py:110-160).  Returns the
        `DeviceTrace`; a previously bound trace is replaced."""
        from ..trace import DeviceTrace

        trace = DeviceTrace(self, signals, every=every, capacity=capacity, envs=envs, wire_temperature=wire_temperature)
        self._backend.bind_trace(trace.desc)
        self._trace = trace
        return trace

    def bind_rng_replay(self, table) -> None:
        """Validation mode: feed the environments caller-provided variates instead of their Philox streams —
        e.g. the draws a native-seed run of the reference made from its NumPy ``Generator(PCG64)``
        (``env.np_random``; call sites ignition.py:233,239,261,327, material.py:127).  ``table`` is
        ``float64[n_steps, 5]`` (the same variates for every environment) or ``float64[n_steps, 5, num_envs]``:
        per physics step since the reset the debris-short roll, the random-short roll, the ignition roll, the
        spark location [mm] and the crater volume [um^3], NaN where nothing is drawn (`_abi.REPLAY_SLOTS`).
        ``None`` returns to Philox.  Runs on the global-memory kernel."""
        if table is None:
            self._backend.bind_rng_replay(None, 0)
            self._replay = None
            return
        t = torch.as_tensor(table, dtype=torch.float64)
        if t.dim() == 2:
            t = t.unsqueeze(-1).expand(-1, -1, self.num_envs)
        if t.dim() != 3 or t.shape[1] != _abi.REPLAY_SLOTS or t.shape[2] != self.num_envs:
            raise ValueError(f"table must be [n_steps, {_abi.REPLAY_SLOTS}] or [n_steps, {_abi.REPLAY_SLOTS}, num_envs]")
        buf = torch.full((t.shape[0], _abi.REPLAY_SLOTS, self.state.stride), float("nan"), dtype=torch.float64,
                         device=self.device)
        buf[:, :, : self.num_envs] = t.to(self.device)
        self._replay = buf  # keep alive: the library only borrows the pointer
        self._backend.bind_rng_replay(buf.data_ptr(), int(t.shape[0]))

    def unbind_trace(self) -> None:
        self._backend.bind_trace(None)
        self._trace = None

    # ---- per-environment physics parameters (domain randomisation) ---------------------------------
    def _envp_consts(self) -> Dict[str, float]:
        return {"base_flow_rate": float(self.dielectric_params.base_flow_rate), "dt_s": float(self.params.dt_s)}

    def _init_env_params(self, values: Dict[str, Any], stride: int) -> None:
        n = self.num_envs
        uni = envp.uniform_values(self)
        cols = {name: np.full(stride, uni[name], dtype=np.float64) for name in envp.NAMES}
        for name, v in values.items():
            a = envp.host_column(name, v, n)
            cols[name][:n] = a
            cols[name][n:] = a[-1]  # padding columns repeat the last environment
        self.env_param_names = tuple(name for name in envp.NAMES if name in values)
        self._envp_src = torch.from_numpy(np.stack([cols[name] for name in envp.NAMES])).to(self.device)
        self._envp_rows = torch.from_numpy(envp.derive_rows(cols, self._envp_consts())).to(self.device)

    def set_env_params(self, values: Dict[str, Any], mask=None) -> None:
        """New values of randomised physics parameters (names given at construction), taking effect at the next launch.
        A value is a scalar or one value per environment; `mask` (bool per environment) limits the change to the
        environments where it is set.  Device tensors are applied on the device with no host synchronisation (and are not
        checked for finiteness); host values are checked and derived in Python floats (see `sparc_amd.core.env_params`)."""
        if self._envp_rows is None:
            raise RuntimeError("construct the environment with env_params={...} to randomise physics parameters")
        values = dict(values)
        envp.check_names(values)
        outside = sorted(set(values) - set(self.env_param_names))
        if outside:
            raise ValueError(f"{outside} not randomised in this environment (env_params named {list(self.env_param_names)})")
        n = self.num_envs
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).reshape(-1).to(torch.bool)
            if m.shape != (n,):
                raise ValueError(f"mask must have one entry per environment ({n})")
        src = {name: self._envp_src[envp.INDEX[name], :n] for name in envp.NAMES}
        host = {}
        new = {}
        for name, v in values.items():
            if torch.is_tensor(v) and v.device.type != "cpu":
                col = v.detach().to(device=self.device, dtype=torch.float64).reshape(-1)
                if col.numel() == 1:
                    col = col.expand(n)
                if col.shape != (n,):
                    raise ValueError(f"env_params[{name!r}] must be a scalar or have one value per environment ({n})")
            else:
                host[name] = envp.host_column(name, v, n)
                col = torch.from_numpy(host[name]).to(self.device)
            new[name] = col
        src.update(new)
        consts = self._envp_consts()
        rows = sorted({r for name in new for r in envp.AFFECTS[name]})
        for r in rows:
            if r == _abi.ENVP.STIFFNESS_COEFF and "omega_n" in host:  # C pow, element by element (module docstring)
                val = torch.from_numpy(envp.derive_row(r, host, consts)).to(self.device)
            else:
                val = envp.derive_row(r, src, consts)
            dst = self._envp_rows[r, :n]
            dst.copy_(val if m is None else torch.where(m, val, dst))
        for name, col in new.items():
            dst = self._envp_src[envp.INDEX[name], :n]
            dst.copy_(col if m is None else torch.where(m, col, dst))

    def get_env_params(self) -> Dict[str, torch.Tensor]:
        """Every randomisable physics parameter per environment (float64 [num_envs] copies, in the dataclass units): the
        environment's own values for the randomised names, the uniform dataclass value for the others."""
        if self._envp_src is None:
            raise RuntimeError("construct the environment with env_params={...} to randomise physics parameters")
        return {name: self._envp_src[envp.INDEX[name], : self.num_envs].clone() for name in envp.NAMES}

    # ---- per-environment wire material (domain randomisation) --------------------------------------
    def _init_wire_material(self, h, d, index: np.ndarray, stride: int) -> None:
        """Every material's full row set, built once: the float64 geometry rows with that material's K_COND / TUF
        ([M, GEOM_F64_COUNT, stride]) and its five material rows ([M, WMAT_COUNT, stride]).  A switch is a device-side
        column select from these tables (`set_wire_material`): exact by construction, no arithmetic."""
        M = len(self.wire_materials)
        mats = [derive.material_rows(self.wire_materials, np.full(self.num_envs, k), self.wire_params, stride) for k in range(M)]
        self._wmat_table = torch.from_numpy(np.stack(mats)).to(self.device)
        self._wmat_index = torch.zeros(stride, dtype=torch.int64, device=self.device)
        self._wmat_rows = torch.empty((_abi.WMAT_COUNT, stride), dtype=torch.float64, device=self.device)
        if self._dyn is not None:
            # dynamic geometry: no row table at a fixed height (it would overwrite the heights); the constructor derived the
            # geometry rows with each environment's material, later switches re-derive them (`set_wire_material`)
            self._wmat_geom_table = None
            self._wmat_index[: self.num_envs].copy_(torch.from_numpy(np.asarray(index, dtype=np.int64)))
            self._select_wire_material_rows(geometry=False)
            return
        geom = [derive.geometry_rows(h, d, self.wire_params, m, self.material_params, stride)[0] for m in self.wire_materials]
        self._wmat_geom_table = torch.from_numpy(np.stack(geom)).to(self.device)
        self.set_wire_material(index)

    def set_wire_material(self, index, mask=None) -> None:
        """Move environments to other materials of ``env.wire_materials``, taking effect at the next launch.  ``index`` is a
        scalar or one index per environment (host values or a device tensor); ``mask`` (bool per environment) limits the
        change to the environments where it is set.  The wire temperatures, and every other state, carry over: a switch
        in mid-episode steps on from the current state with the new material's constants.  Host indices are checked;
        device tensors are applied on the device with no host synchronisation -- an entry outside ``[0,
        len(wire_materials))`` there leaves its environment's material as it was.  In a ``dynamic_geometry`` environment the
        geometry rows of the masked environments are derived again from their stored heights and diameter indices with the
        new material (`sparc_amd.geometry`): the heights survive the switch."""
        if self._wmat_rows is None:
            raise RuntimeError("construct the environment with wire_material=[...] to give environments their own wire material")
        n, M = self.num_envs, len(self.wire_materials)
        if torch.is_tensor(index) and index.device.type != "cpu":
            idx = index.detach().to(device=self.device, dtype=torch.int64).reshape(-1)
            if idx.numel() == 1:
                idx = idx.expand(n)
            if idx.shape != (n,):
                raise ValueError(f"wire material index must be a scalar or have one entry per environment ({n})")
            idx = torch.where((idx >= 0) & (idx < M), idx, self._wmat_index[:n])
        else:
            a = np.asarray(index.detach().numpy() if torch.is_tensor(index) else index).reshape(-1)
            if a.size == 1:
                a = np.broadcast_to(a, (n,))
            if a.shape != (n,):
                raise ValueError(f"wire material index must be a scalar or have one entry per environment ({n})")
            if not np.issubdtype(a.dtype, np.integer):
                raise ValueError("wire material index must be integers")
            if a.min() < 0 or a.max() >= M:
                raise ValueError(f"wire material index out of range [0, {M}) (env.wire_materials: "
                                 f"{[m.name for m in self.wire_materials]})")
            idx = torch.from_numpy(a.astype(np.int64)).to(self.device)
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).reshape(-1).to(torch.bool)
            if m.shape != (n,):
                raise ValueError(f"mask must have one entry per environment ({n})")
            idx = torch.where(m, idx, self._wmat_index[:n])
        self._wmat_index[:n].copy_(idx)
        self._select_wire_material_rows(mask=mask)

    def _select_wire_material_rows(self, mask=None, geometry: bool = True) -> None:
        """The geometry and material rows of the current material index, selected from the fixed per-material tables.  With
        ``dynamic_geometry`` only the material rows are selected; the geometry rows (of the masked environments) are derived
        again from the stored heights and diameter indices, unless ``geometry`` is False."""
        n, cur = self.num_envs, self._wmat_index
        cur[n:].copy_(cur[n - 1: n].expand(cur.shape[0] - n))  # padding columns repeat the last environment
        tables = ((self._wmat_table, self._wmat_rows),) if self._dyn is not None else \
            ((self._wmat_geom_table, self._geom_f64), (self._wmat_table, self._wmat_rows))
        for table, dst in tables:
            dst.copy_(torch.gather(table, 0, cur.view(1, 1, -1).expand(1, table.shape[1], -1))[0])
        if self._dyn is not None and geometry:
            _geometry.rederive(self, mask)

    # ---- per-episode workpiece height and wire diameter (sparc_amd.geometry) ----------
    def set_geometry(self, workpiece_height=None, wire_diameter_index=None, mask=None, reset: bool = True) -> None:
        """New workpiece heights [mm] and / or wire diameters (indices into ``dynamic_geometry``'s ``wire_diameters``) for the
        environments where ``mask`` (bool per environment; default: all) is set.  A value is a scalar, one value per
        environment (sequence, NumPy array) or a device tensor.  The values are merged under the mask on the device, the
        geometry rows derived by one launch (`wedm_derive_geometry`) with the bits the host derivation writes, and with
        ``reset=True`` the masked environments are reset: a new workpiece is a new episode (the wire's length follows the
        height).  ``reset=False`` is for a caller whose next launch resets exactly those environments itself, as
        `WireEDMVectorEnv` does; stepping an environment on with rows of another height is not a defined simulation.
        Nothing is read back: a height that is NaN, infinite, not positive or above ``max_workpiece_height`` and an index
        outside the list leave that environment's geometry as it was, and `check_errors` raises for them."""
        _geometry.set_geometry(self, workpiece_height, wire_diameter_index, mask, reset)

    def get_geometry(self) -> Dict[str, torch.Tensor]:
        """Each environment's current ``workpiece_height`` [mm] (float64), ``wire_diameter`` [mm] (float64) and
        ``n_segments`` (int32: the cells of its wire), as device copies.  Needs ``dynamic_geometry``."""
        return _geometry.get_geometry(self)

    def get_wire_material_index(self) -> torch.Tensor:
        """Each environment's current material, an index into ``env.wire_materials`` (int64 [num_envs] device copy)."""
        if self._wmat_rows is None:
            raise RuntimeError("construct the environment with wire_material=[...] to give environments their own wire material")
        return self._wmat_index[: self.num_envs].clone()

    # ---- checkpoint / resume (the reference has none for simulation state) ---------
    def _physics_fingerprint(self) -> str:
        """sha256 over everything that determines the physics of a continuation: the whole
        `wedm_params` block the kernels receive (configuration, module parameters, derived constants,
        control mode, shard offset) and, with per-environment geometry, the geometry rows -- with
        per-environment wire material the fixed per-material row table instead of the current float64
        rows, which change when an environment switches material (the choice is checkpointed itself)."""
        import ctypes
        import hashlib

        h = hashlib.sha256(ctypes.string_at(ctypes.addressof(self.params), ctypes.sizeof(self.params)))
        if self._dyn is not None:  # capacity, catalogue and table: the current rows change with every episode
            h.update(self._dyn.fingerprint())
            if self._wmat_rows is not None:
                h.update(self._wire_material_fingerprint().encode())
        elif self.per_env_geometry:
            if self._wmat_rows is not None:
                h.update(self._wire_material_fingerprint().encode())
            else:
                h.update(self._geom_f64.cpu().numpy().tobytes())
            h.update(self._geom_i32.cpu().numpy().tobytes())
        return h.hexdigest()

    def _wire_material_fingerprint(self) -> str:
        import hashlib

        h = hashlib.sha256(self._dyn.combo_host.tobytes() if self._dyn is not None
                           else self._wmat_geom_table.cpu().numpy().tobytes())
        h.update(self._wmat_table.cpu().numpy().tobytes())
        return h.hexdigest()

    def state_dict(self) -> Dict[str, Any]:
        """Everything a bit-identical continuation needs: the raw state blocks (Philox key, episode
        and clocks live in them, so the random streams resume exactly), the reset seed, and a
        fingerprint of the physics parameters (tensors, ints and strings only: loads with
        ``weights_only=True``)."""
        return {"abi_version": _abi.ABI_VERSION, "blocks": self.state.clone_blocks(), "seed": self._seed, "num_envs": self.num_envs,
                "n_segments": self.n_segments, "env_id_offset": self.env_id_offset, "pulse_stats": self.pulse_stats,
                "signal_stats": self.signal_stats,
                "steps_since_reset": self.steps_since_reset, "physics": self._physics_fingerprint(),
                **self._env_params_state(), **self._wire_material_state(), **_geometry.state(self)}

    def _wire_material_state(self) -> Dict[str, Any]:
        if self._wmat_rows is None:
            return {"wire_materials": None}
        return {"wire_materials": [m.name for m in self.wire_materials], "wire_material_table": self._wire_material_fingerprint(),
                "wire_material_index": self._wmat_index[: self.num_envs].detach().cpu().clone()}

    def _env_params_state(self) -> Dict[str, Any]:
        if self._envp_rows is None:
            return {"env_param_names": None}
        return {"env_param_names": list(self.env_param_names), "env_params_src": self._envp_src.detach().cpu().clone(),
                "env_params_rows": self._envp_rows.detach().cpu().clone()}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        if sd.get("abi_version") != _abi.ABI_VERSION:
            raise ValueError(f"checkpoint was written with state layout ABI {sd.get('abi_version', '<= 3')}, this build is ABI "
                             f"{_abi.ABI_VERSION} (rows and the wire-temperature layout differ): it cannot be continued here")
        if (sd["num_envs"], sd["n_segments"], sd["env_id_offset"]) != (self.num_envs, self.n_segments, self.env_id_offset):
            raise ValueError("checkpoint was taken from an environment of a different shape / shard")
        if bool(sd.get("pulse_stats", False)) != self.pulse_stats:
            raise ValueError(f"checkpoint was taken with pulse_stats={bool(sd.get('pulse_stats', False))}, this environment has "
                             f"pulse_stats={self.pulse_stats}: the observation and the interval counts differ")
        if bool(sd.get("signal_stats", False)) != self.signal_stats:
            raise ValueError(f"checkpoint was taken with signal_stats={bool(sd.get('signal_stats', False))}, this environment "
                             f"has signal_stats={self.signal_stats}: the observation and the interval sums differ")
        mine = list(self.env_param_names) if self._envp_rows is not None else None
        theirs = sd.get("env_param_names")
        if (list(theirs) if theirs is not None else None) != mine:
            raise ValueError(f"checkpoint was taken with per-environment physics parameters {theirs}, this environment "
                             f"randomises {mine}")
        mine_m = [m.name for m in self.wire_materials] if self._wmat_rows is not None else None
        theirs_m = sd.get("wire_materials")
        if (list(theirs_m) if theirs_m is not None else None) != mine_m or \
                (mine_m is not None and sd.get("wire_material_table") != self._wire_material_fingerprint()):
            raise ValueError(f"checkpoint was taken with per-environment wire materials {theirs_m}, this environment has "
                             f"{mine_m}" + (" (same names, different constants or geometry)" if theirs_m == mine_m else "")
                             + ": the material table differs")
        _geometry.check_state(self, sd)
        if sd.get("physics") != self._physics_fingerprint():
            raise ValueError("checkpoint was taken with different physics (configuration, module parameters, control "
                             "mode or per-environment geometry): continuing would silently change the trajectory")
        if mine is not None:
            for key, dst in (("env_params_src", self._envp_src), ("env_params_rows", self._envp_rows)):
                if tuple(sd[key].shape) != tuple(dst.shape):
                    raise ValueError(f"checkpoint block {key!r} has shape {tuple(sd[key].shape)}, this environment's is "
                                     f"{tuple(dst.shape)}")
        if mine_m is not None:
            idx = sd["wire_material_index"]
            if tuple(idx.shape) != (self.num_envs,):
                raise ValueError(f"checkpoint block 'wire_material_index' has shape {tuple(idx.shape)}, expected ({self.num_envs},)")
        self.state.load_blocks(sd["blocks"])
        if mine is not None:
            self._envp_src.copy_(sd["env_params_src"])
            self._envp_rows.copy_(sd["env_params_rows"])
        _geometry.load_state(self, sd)  # heights and indices; the rows are derived from them (below, where materials differ)
        if mine_m is not None:
            self.set_wire_material(sd["wire_material_index"].numpy())
        self._seed = int(sd["seed"])
        self.steps_since_reset = int(sd["steps_since_reset"])

    # ---- snapshot / restore / fork of environment subsets, on the device (sparc_amd.snapshot) ----
    def snapshot(self, env_ids=None) -> "_snapshot.EnvSnapshot":
        """Compact device copies of the state of the environments ``env_ids`` (default: all; a source may be named more
        than once): their columns of every state block -- ``f64``, ``i32``, ``i8``, ``T``, ``obs``, ``stats``, ``reward``
        and, where present, ``crater_log``, ``pulse``, ``signal`` -- with ``env_params=`` their parameter values and
        derived rows, with ``wire_material=`` their material index; one launch, no temporaries.  Not in it: the trace
        ring, the injected-variate table, ``steps_since_reset`` and the geometry (it belongs to the slot).
        Indices are a Python sequence, a NumPy array or a tensor.  Host indices are checked here.  A device tensor is not
        read back (its range is checked by the kernel and reported by `check_errors`), except on an environment whose
        slots differ in ``(height, diameter)``, where every call reads the indices once (a synchronisation)."""
        return _snapshot.snapshot(self, env_ids)

    def restore(self, snap, env_ids=None, columns=None) -> None:
        """Snapshot column ``columns[i]`` into environment ``env_ids[i]``.  Defaults: ``columns`` = ``0 .. len(env_ids) - 1``
        (all of them without ``env_ids``), ``env_ids`` = the environments those columns were taken from.  Raises
        ``ValueError`` for a snapshot of another ABI version, shape (segments, observation, crater-log capacity), block
        set, physics fingerprint or material table, for indices out of range, a destination named twice, and a column
        whose slot had another ``(height, diameter)`` than its destination.  With ``env_params=`` the parameter rows are
        written, with ``wire_material=`` the material index, after which the rows are selected as `set_wire_material`
        does.  A restore into the slot a column came from replays exactly (`fork` on the random stream).  Index forms
        and their checks: see `snapshot`; for device tensors a duplicate destination is found on the device too."""
        _snapshot.restore(self, snap, env_ids, columns)

    def fork(self, src_ids, dst_ids) -> None:
        """Environment ``dst_ids[i]`` becomes a copy of environment ``src_ids[i]``: in place, one launch, no temporaries,
        the same blocks and rows as `snapshot` followed by `restore`.  One source may feed many destinations and a single
        ``src_ids`` serves all; sources must not be among the destinations and destinations must be distinct
        (``ValueError`` for host indices; for device tensors a flag that `check_errors` raises for).
        The random stream: the Philox key and the episode are state and are copied; the counter also holds the SLOT's
        global id (``env_id_offset`` + index), which is not.  A fork into another slot therefore continues with that
        slot's own variates -- an independent sample of the same state, which is what shooting and tree search want --
        while a restore into the slot the state came from replays bit for bit."""
        _snapshot.fork(self, src_ids, dst_ids)

    def save_checkpoint(self, path) -> None:
        torch.save(self.state_dict(), path)

    def load_checkpoint(self, path) -> None:
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))

    def wire_profile(self, bins: int = 8, env_ids=None) -> Dict[str, torch.Tensor]:
        """The wire's temperature profile per environment, for any geometry, by one launch on the device: float32 tensors
        ``zone_mean``, ``wire_mean``, ``wire_max``, ``hot_cell`` of shape ``[count]`` (the mean over the environment's
        workpiece zone, the mean and maximum over its wire, the lowest index of the hottest cell), ``bin_max`` /
        ``bin_mean`` of shape ``[bins, count]`` (the wire pooled into ``bins`` bins: bin ``b`` covers the cells
        ``[b * n // bins, (b + 1) * n // bins)``, at least one), and ``rows``, the ``[4 + 2 * bins, count]`` block they are
        views of.  Means are float64 sums rounded once.  The tensors are valid until the next call with the same
        ``(bins, count)``; indices may be a device tensor (never read back, mistakes reach `check_errors`).  See
        `sparc_amd.profile.wire_profile` and DESIGN.md section 4.12."""
        return _profile.wire_profile(self, bins, env_ids)

    def zone_mean_temperature(self) -> torch.Tensor:
        """Mean wire temperature over the workpiece zone (wire.py:390-398), per environment.  With per-environment geometry
        (``workpiece_height=`` / ``wire_diameter=`` / ``wire_material=``) every environment's own zone, from `wire_profile`."""
        if self.geometry is None:
            return self.wire_profile(bins=0)["zone_mean"].clone()
        g = self.geometry
        lo, hi = g.az_start, g.az_end
        T = self.state.wire_temperature.tensor().t()  # [segment, env], as the reduction was written for ABI v3
        if hi > lo:
            return T[lo:hi].mean(dim=0)
        return T[: g.n_seg].mean(dim=0)

    # ---- statistics the reference's modules expose -------------------------
    def get_short_circuit_status(self) -> Dict[str, torch.Tensor]:
        """`IgnitionModule.get_short_circuit_status` (ignition.py:386-399), per environment."""
        r, d = self.state.random_short_remaining, self.state.debris_short_remaining
        return {"has_random_short": r > 0, "random_short_remaining_us": r, "has_debris_short": d > 0,
                "debris_short_remaining_us": d, "total_short_remaining_us": torch.maximum(r, d)}

    def get_debris_statistics(self) -> Dict[str, torch.Tensor]:
        """`DielectricModule.get_debris_statistics` (dielectric.py:174-182), per environment."""
        st = self.state
        return {"debris_volume_mm3": st.debris_volume, "debris_density": st.debris_density,
                "cavity_volume_mm3": st.cavity_volume, "flow_condition": st.flow_rate,
                "debris_fill_percentage": st.debris_density * 100.0}

    def get_crater_statistics(self) -> Dict[str, torch.Tensor]:
        """`MaterialRemovalModule.get_crater_statistics` (material.py:207-227), per environment, from
        the running sum / sum of squares / min / max the kernels keep at every fresh spark (the
        list of all volumes, ``volumes_um3``, is not kept; trace ``last_crater_volume`` to get it).
        Zeros while an environment has had no crater, as in the reference."""
        from .._abi import STAT

        st, n = self.state.stats[:, : self.num_envs], self.state.spark_count
        none = n == 0
        denom = torch.clamp(n, min=1).to(torch.float64)
        mean = st[STAT.CRATER_SUM] / denom
        var = torch.clamp(st[STAT.CRATER_SUMSQ] / denom - mean * mean, min=0.0)
        zero = torch.zeros_like(mean)
        return {"total_craters": n, "mean_volume_um3": mean, "std_volume_um3": torch.sqrt(var),
                "min_volume_um3": torch.where(none, zero, st[STAT.CRATER_MIN]),
                "max_volume_um3": torch.where(none, zero, st[STAT.CRATER_MAX])}

    def get_pulse_statistics(self) -> Dict[str, torch.Tensor]:
        """The reference driver's "Sparks" and "Short pulses" (experiments/run_simulation.py:597-636) of the last completed
        control interval, per environment, as the kernels published them at its control step: ``spark_pulses`` /
        ``short_pulses`` = rising edges of ``current > 0.1`` A outside / inside a short circuit, ``short_steps`` = physics
        steps with ``is_short_circuit`` (int32 views; zeros until the first control step after a reset).  Summing the
        published counts of the last 200 intervals gives the driver's "Last 200ms" figures.  Needs ``pulse_stats=True``."""
        rows = self.state.pulse
        if rows is None:
            raise RuntimeError("construct the environment with pulse_stats=True to count pulses")
        P = _abi.PULSE
        n = self.num_envs
        return {"spark_pulses": rows[P.SPARK_LAST, :n], "short_pulses": rows[P.SHORT_LAST, :n],
                "short_steps": rows[P.SHORT_STEPS_LAST, :n]}

    def get_signal_statistics(self) -> Dict[str, torch.Tensor]:
        """What went into the gap over the last completed control interval, per environment, as the kernels published it at
        its control step (float64; zeros until the first control step after a reset): ``samples`` = physics steps the
        environment ran in the interval, ``current_sum`` [A], ``energy_sum`` [V A] and ``gap_sum`` [um] over them,
        ``gap_min`` [um] and ``tmax_peak`` their extrema; ``mean_current``, ``mean_power`` and ``mean_gap`` = the sums
        divided by ``samples`` (0 where there were none).  Needs ``signal_stats=True``."""
        rows = self.state.signal
        if rows is None:
            raise RuntimeError("construct the environment with signal_stats=True to keep the interval's signal statistics")
        S = _abi.SIG
        n = self.num_envs
        samples = rows[S.SAMPLES_LAST, :n]
        out = {"samples": samples, "current_sum": rows[S.CURRENT_LAST, :n], "energy_sum": rows[S.ENERGY_LAST, :n],
               "gap_sum": rows[S.GAP_LAST, :n], "gap_min": rows[S.GAP_MIN_LAST, :n], "tmax_peak": rows[S.TMAX_PEAK_LAST, :n]}
        none = samples == 0
        denom = torch.where(none, torch.ones_like(samples), samples)
        zero = torch.zeros_like(samples)
        for mean, total in (("mean_current", "current_sum"), ("mean_power", "energy_sum"), ("mean_gap", "gap_sum")):
            out[mean] = torch.where(none, zero, out[total] / denom)
        return out

    def get_crater_volumes(self, env_index: int) -> torch.Tensor:
        """`MaterialRemovalModule.crater_volumes_um3` (material.py:133) of one environment since its reset, oldest
        first, from the ring the kernels fill at every fresh spark (needs ``crater_log_capacity``; when more craters
        were sampled than the ring holds, the newest ``capacity`` of them)."""
        log = self.state.crater_log
        if log is None:
            raise RuntimeError("construct the environment with crater_log_capacity > 0 to keep the crater volumes")
        n, cap = int(self.state.spark_count[env_index].item()), log.shape[0]
        if n <= cap:
            return log[:n, env_index].clone()
        idx = torch.arange(n - cap, n, device=log.device) % cap
        return log[idx, env_index]

    def get_crater_count(self) -> torch.Tensor:
        """`len(MaterialRemovalModule.crater_volumes_um3)` (material.py:133), per environment."""
        return self.state.spark_count

    @property
    def workpiece_height(self) -> float:
        return self.config.workpiece_height

    @property
    def wire_diameter(self) -> float:
        return self.config.wire_diameter



def _material_table(wire_material, n: int, table=None):
    """(materials of ``env.wire_materials``, int64 index per environment) of a ``wire_material=`` argument.  ``table``: the
    materials in a fixed order (``wire_material_table=``; every entry must be one of them); default: the distinct ones, in
    order of first appearance."""
    from ..core.material_db import WireMaterial

    if isinstance(wire_material, (str, WireMaterial)):
        raise ValueError(f"wire_material must be a sequence of num_envs={n} names or WireMaterial objects "
                         f"(one material for the whole batch: EnvironmentConfig(wire_material=...))")
    items = list(wire_material)
    if len(items) != n:
        raise ValueError(f"wire_material has {len(items)} entries, expected one per environment ({n})")
    db = get_material_db()
    fixed = table is not None
    table = [] if table is None else [db.get_wire_material(str(m)) if isinstance(m, (str, np.str_)) else m for m in table]
    keys = {}
    for k, m in enumerate(table):
        if not isinstance(m, WireMaterial):
            raise ValueError(f"wire_material_table[{k}] must be a material name or a WireMaterial, got {type(m).__name__}")
        if any(o.name == m.name for o in table[:k]):
            raise ValueError(f"wire_material_table names {m.name!r} twice")
        keys[dataclasses.astuple(m)] = k
    index = np.empty(n, dtype=np.int64)
    seen = {}  # id of an item object / a name -> table index (one lookup per distinct item, not per environment)
    for e, item in enumerate(items):
        tag = str(item) if isinstance(item, (str, np.str_)) else id(item)
        k = seen.get(tag)
        if k is None:
            if isinstance(item, WireMaterial):
                mat = item
            elif isinstance(item, (str, np.str_)):
                mat = db.get_wire_material(str(item))
            else:
                raise ValueError(f"wire_material[{e}] must be a material name or a WireMaterial, got {type(item).__name__}")
            key = dataclasses.astuple(mat)
            k = keys.get(key)
            if k is None:
                if fixed:
                    raise ValueError(f"wire_material[{e}] ({mat.name!r}) is not in wire_material_table "
                                     f"{[m.name for m in table]}")
                if any(m.name == mat.name for m in table):
                    raise ValueError(f"wire_material names two different materials {mat.name!r}")
                k = keys[key] = len(table)
                table.append(mat)
            seen[tag] = k
        index[e] = k
    return tuple(table), index


def _to_numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
