"""Gymnasium-VectorEnv-style adapter with automatic reset.

The reference leaves observation and reward as TODOs (`envs/wire_edm.py:100-101,181-187`) and
has no vector API; this adapter gives RL code the usual contract on top of the batched
environment: `step()` advances one control interval (one fused launch), returns
`(obs, reward, terminated, truncated, info)` with a leading batch dimension, and environments
that terminated are reset at the start of the next `step()` ("next-step" autoreset), each with a
fresh Philox episode stream.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .envs.wire_edm import WireEDMEnv
from .reward import ShapedReward


def progress_reward(env: WireEDMEnv, prev: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Default reward of the adapter (the reference's `_calculate_reward` is a TODO returning 0.0,
    envs/wire_edm.py:185-187): micrometres cut during the control interval, minus 10 when the wire
    broke or collided in it, float32 per environment."""
    st = env.state
    cut = (st.workpiece_position - prev["workpiece_position"]).to(torch.float32)
    return cut - 10.0 * st.is_wire_broken.to(torch.float32)


def uniform_param_sampler(ranges: Dict[str, Tuple[float, float]], generator: Optional[torch.Generator] = None):
    """A `param_sampler` for `WireEDMVectorEnv`: every named physics parameter uniform in ``[low, high)``, drawn on the
    environment's device (``generator`` must live there when given).  ``omega_n`` draws keep 26 significant bits, so that
    the stiffness row derived on the device equals Python's ``omega_n ** 2`` (`sparc_amd.core.env_params`)."""
    spec = {name: (float(lo), float(hi)) for name, (lo, hi) in ranges.items()}
    for name, (lo, hi) in spec.items():
        if not (lo <= hi):
            raise ValueError(f"range of {name!r} must have low <= high, got ({lo}, {hi})")

    def sample(env: WireEDMEnv, reset_mask: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for name, (lo, hi) in spec.items():
            u = torch.rand(env.num_envs, generator=generator, device=env.device, dtype=torch.float64)
            x = lo + (hi - lo) * u
            if name == "omega_n":  # clear the low 27 of 52 mantissa bits
                x = (x.view(torch.int64) & ~((1 << 27) - 1)).view(torch.float64)
            out[name] = x
        return out

    return sample


def uniform_material_sampler(generator: Optional[torch.Generator] = None):
    """A `material_sampler` for `WireEDMVectorEnv`: every environment draws one of ``env.wire_materials`` uniformly, on the
    environment's device (``generator`` must live there when given)."""

    def sample(env: WireEDMEnv, reset_mask: torch.Tensor) -> torch.Tensor:
        return torch.randint(0, len(env.wire_materials), (env.num_envs,), generator=generator, device=env.device,
                             dtype=torch.int64)

    return sample


def uniform_geometry_sampler(height: Optional[Tuple[float, float]] = None, diameters: bool = True,
                             generator: Optional[torch.Generator] = None):
    """A `geometry_sampler` for `WireEDMVectorEnv`: the workpiece height uniform in ``[low, high)`` [mm] (``height=None``:
    heights stay) and, with ``diameters=True``, one of the environment's ``dynamic_geometry`` wire diameters uniformly, drawn
    on the environment's device (``generator`` must live there when given)."""
    if height is not None:
        lo, hi = float(height[0]), float(height[1])
        if not (0.0 < lo <= hi):
            raise ValueError(f"height range must have 0 < low <= high, got ({lo}, {hi})")

    def sample(env: WireEDMEnv, reset_mask: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        if height is not None:
            out["workpiece_height"] = lo + (hi - lo) * torch.rand(env.num_envs, generator=generator, device=env.device,
                                                                  dtype=torch.float64)
        if diameters:
            out["wire_diameter_index"] = torch.randint(0, len(env._dyn.diameters), (env.num_envs,), generator=generator,
                                                       device=env.device, dtype=torch.int64)
        return out

    return sample


class WireEDMVectorEnv:
    """Next-step autoreset (Gymnasium's ``AutoresetMode.NEXT_STEP``): the `step()` after the one that
    reported ``terminated`` / ``truncated`` for an environment starts a new episode for it.

    When the wrapped environment was built with ``autoreset=True`` the reset happens INSIDE the step
    kernel (`wedm_params.autoreset`, include/wedm_hip.h): an environment found terminated when the
    launch begins is re-initialised by that launch and stepped on, and with ``reward="progress"`` the
    kernel also writes the reward — `step()` is then exactly one kernel launch and no device-to-host
    read.  Otherwise (or with a callable reward) the adapter falls back to a masked `reset` launch and
    a torch expression."""

    def __init__(self, env: WireEDMEnv, *, max_episode_steps: Optional[int] = None, autoreset: bool = True,
                 reward=None, param_sampler: Optional[Callable] = None, material_sampler: Optional[Callable] = None,
                 wire_profile_bins: Optional[int] = None, geometry_sampler: Optional[Callable] = None,
                 episode_sampler=None, normalizer=None, episode_log=None, sensor=None):
        """``reward``: None keeps the environment's own reward (the reference's constant 0.0, or the
        in-kernel progress reward if the environment was built with ``reward="progress"``);
        ``"progress"`` selects `progress_reward` (computed in the kernel when the environment supports
        it); a callable ``f(env, prev) -> float32[N]`` receives the environment after the control
        interval and ``prev = {"workpiece_position": ...}`` snapshotted before it (all on the device); a
        `sparc_amd.reward.ShapedReward` is a weighted sum of ten terms of the step -- progress, a cost per step, wire break,
        target, the step's sparks, shorts and short-circuit samples, its energy, the gap below a floor, the peak temperature
        above a ceiling -- formed by one `wedm_reward` call after the launch (one copy of a row before it; no host
        synchronisation, no allocation after the first step) from the accumulator rows, which hold what this step's action
        caused; ``info["reward_terms"]`` is the float64 ``[10, N]`` block of the weighted terms, valid until the next step,
        the normaliser and the episode log take the shaped reward as the raw reward, and the environment's own reward row is
        ignored.
        ``param_sampler``: domain randomisation -- ``f(env, reset_mask) -> {name: float64[N] device tensor}`` is called at
        every `step()` before the launch (and at `reset()` with every environment marked); the values are applied
        (`WireEDMEnv.set_env_params`) only where ``reset_mask`` is set, so each new episode starts with freshly drawn
        physics.  The environment must have been built with ``env_params`` naming the sampled parameters
        (see `uniform_param_sampler`).
        ``material_sampler``: the same for the wire material -- ``f(env, reset_mask) -> int64[N] device tensor`` of indices
        into ``env.wire_materials``, applied (`WireEDMEnv.set_wire_material`) where ``reset_mask`` is set, at the same
        point as ``param_sampler``.  The environment must have been built with ``wire_material=[...]`` (see
        `uniform_material_sampler`).
        ``geometry_sampler``: the same for the workpiece height and the wire diameter -- ``f(env, reset_mask) ->
        {"workpiece_height": float64[N], "wire_diameter_index": int64[N]}`` (device tensors, either key optional), applied
        (`WireEDMEnv.set_geometry` with ``reset=False``: the reset is this adapter's) where ``reset_mask`` is set, before the
        other two samplers (the material sampler's re-derivation reads the heights).  The environment must have been built
        with ``dynamic_geometry={...}`` (see `uniform_geometry_sampler`).
        ``episode_sampler``: a `sparc_amd.randomize.EpisodeSampler` -- seeded domain randomisation of all of the above by one
        device launch, each draw a pure function of (seed, global environment id, draw number), applied where the three
        samplers would be.  It excludes them.  ``reset(seed=x)`` reseeds it with ``x``; a seed together with a mask is
        refused (it would put the unmasked environments' draws on another seed's sequence).
        ``wire_profile_bins``: with an integer B in [0, 64], `reset()` and `step()` return ``[N, obs_dim + 4 + 2 * B]``: the
        environment's observation followed by the rows of `WireEDMEnv.wire_profile` (zone mean, wire mean, maximum,
        hottest cell, B bin maxima, B bin means) of the wire as the launch left it -- one more launch, no host
        synchronisation; `obs_names` and the observation spaces grow to match.
        ``normalizer``: a `sparc_amd.normalize.Normalizer` -- `reset()` and `step()` return the observation (profile columns
        included) standardised by running moments over every environment and step, `step()` the reward scaled by the running
        deviation of the discounted return, by `wedm_normalize` (at most three more launches, no host synchronisation, no
        allocation after the first call); ``info["episode_stats"]`` holds the return ``r`` and length ``l`` of each
        environment's last finished episode, its ``count`` of finished episodes and whether it ``finished`` one in this
        step (device tensors, valid until the next step), ``info["raw_observation"]`` / ``info["raw_reward"]`` the values
        before normalisation.  The normalised tensors are the normaliser's cached outputs: valid until the next call.
        Environments that are frozen during a step (done, with ``autoreset=False``) take no part in the statistics and keep
        their rows; a masked `reset` zeroes the rows of the environments it resets.
        ``episode_log``: a `sparc_amd.episode_log.EpisodeLog` -- `step()` ends with one `wedm_episode_log` call (at most three
        more launches, no host synchronisation, no allocation after binding) that appends a record for every environment
        whose episode ended in the step, in the order of the global environment index, and adds the step to the per-episode
        sums; ``episode_log.read()`` hands the records out when the user chooses.  A frozen environment (done, with
        ``autoreset=False``) is logged once; `reset` zeroes the sums of the environments it resets and logs nothing.
        ``sensor``: a `sparc_amd.sensor.Sensor` -- what `reset()` and `step()` hand out (and what the normaliser reads) is the
        sensor's plane instead of the raw columns: per output channel a raw column delayed, miscalibrated per episode, with
        fresh noise, quantised and saturated, then clean ``priv.<name>`` copies, by one `wedm_sensor` call (no host
        synchronisation, no allocation after binding).  `obs_names`, the observation spaces and ``actor_obs_dim`` (the
        leading measured columns: ``PolicyNet(vec.actor_obs_dim, head)`` reads them in place) become the sensor's;
        ``info["raw_observation"]`` stays the clean full observation.  A frozen environment keeps its last reading."""
        self.env = env
        self.num_envs = env.num_envs
        self.single_action_space = env.single_action_space
        self.single_observation_space = env.single_observation_space
        self.action_space = env.action_space
        self.observation_space = env.observation_space
        self.wire_profile_bins = None
        self.obs_names = tuple(env.obs_names)
        if wire_profile_bins is not None:
            from .envs.wire_edm import Box
            from .profile import _check_bins, profile_names

            self.wire_profile_bins = _check_bins(wire_profile_bins)
            self.obs_names += profile_names(self.wire_profile_bins)
            self.single_observation_space = Box(-np.inf, np.inf, (len(self.obs_names),), np.float32)
            self.observation_space = self.single_observation_space
        self.autoreset = bool(autoreset)
        self.max_episode_steps = max_episode_steps
        self._in_kernel_reset = self.autoreset and bool(getattr(env, "autoreset", False))
        if getattr(env, "autoreset", False) and not self.autoreset:
            raise ValueError("the environment resets terminated environments in the kernel (autoreset=True): "
                             "the adapter cannot switch that off")
        if reward == "progress" and getattr(env, "reward_kind", None) == "progress":
            reward = None  # the kernel writes it
        self._shaped = reward if isinstance(reward, ShapedReward) else None
        if self._shaped is not None:
            reward = None
        self._reward_fn = progress_reward if reward == "progress" else reward
        if self._reward_fn is not None and not callable(self._reward_fn):
            raise ValueError("reward must be None, 'progress' or a callable")
        self._param_sampler = param_sampler
        if param_sampler is not None and getattr(env, "_envp_rows", None) is None:
            raise ValueError("param_sampler needs an environment built with env_params={...} naming the sampled parameters")
        self._material_sampler = material_sampler
        if material_sampler is not None and getattr(env, "_wmat_rows", None) is None:
            raise ValueError("material_sampler needs an environment built with wire_material=[...] listing the materials")
        self._geometry_sampler = geometry_sampler
        if geometry_sampler is not None and getattr(env, "_dyn", None) is None:
            raise ValueError("geometry_sampler needs an environment built with dynamic_geometry={...}")
        self._samples = any(f is not None for f in (param_sampler, material_sampler, geometry_sampler))
        self._episode_sampler = episode_sampler
        if episode_sampler is not None:
            if self._samples:
                raise ValueError("episode_sampler replaces param_sampler / material_sampler / geometry_sampler: give either")
            episode_sampler.bind(env)
        self._need_reset = torch.zeros(self.num_envs, dtype=torch.bool, device=env.device)
        if self._shaped is not None:
            self._shaped.bind(self)
        self.episode_count = torch.zeros(self.num_envs, dtype=torch.int64, device=env.device)
        self.sensor = sensor
        self.raw_obs_names = self.obs_names
        self.actor_obs_dim = len(self.obs_names)
        if sensor is not None:
            from .envs.wire_edm import Box

            sensor.bind(self)  # (against the raw columns, the wire profile's included)
            self.obs_names = tuple(sensor.obs_names)
            self.actor_obs_dim = sensor.actor_dim
            self.single_observation_space = Box(-np.inf, np.inf, (len(self.obs_names),), np.float32)
            self.observation_space = self.single_observation_space
        self.normalizer = normalizer
        if normalizer is not None:
            normalizer.bind(self.obs_names, self.num_envs, env.device, getattr(env, "_backend", None))
        self.episode_log = episode_log
        if episode_log is not None:
            episode_log.bind(self)

    def reset(self, *, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        if self._episode_sampler is not None:
            mask = (options or {}).get("mask")
            if seed is not None:
                if mask is not None:
                    raise ValueError("reset(seed=...) reseeds the episode sampler for every environment: no mask with it")
                self._episode_sampler.reseed(seed)
            self._episode_sampler.draw(self.env, mask=mask, reset=False)
        if self._samples:
            mask = (options or {}).get("mask")
            mask = torch.ones(self.num_envs, dtype=torch.bool, device=self.env.device) if mask is None else \
                torch.as_tensor(mask, device=self.env.device).reshape(-1).to(torch.bool)
            self._apply_sampler(mask)
        obs, info = self.env.reset(seed=seed, options=options)
        self._need_reset.zero_()
        if self.episode_log is not None:
            mask = (options or {}).get("mask")
            if mask is not None:
                mask = torch.as_tensor(mask, device=self.env.device).reshape(-1).to(torch.bool)
            self.episode_log.reset_sums(mask)
        if self.normalizer is not None:
            mask = (options or {}).get("mask")
            if mask is not None:
                mask = torch.as_tensor(mask, device=self.env.device).reshape(-1).to(torch.bool)
            self.normalizer.reset_rows(mask)
            planes = self._planes()
            out, _ = self.normalizer.normalize(self._sensed(planes, None, mask), mask=mask)
            info = dict(info)
            info["raw_observation"] = self._raw(obs, planes)
            return out, info
        if self.sensor is not None:
            mask = (options or {}).get("mask")
            if mask is not None:
                mask = torch.as_tensor(mask, device=self.env.device).reshape(-1).to(torch.bool)
            planes = self._planes()
            info = dict(info)
            info["raw_observation"] = self._raw(obs, planes)
            return self._sensed(planes, None, mask)[0].t().contiguous(), info
        return self._observation(obs), info

    def _sensed(self, planes, first, mask):
        """The planes in front of the normaliser: the sensor's output plane where there is a sensor (one `wedm_sensor` call
        with the episode numbers as they stand), else ``planes`` themselves."""
        if self.sensor is None:
            return planes
        return [self.sensor.apply(planes, first=first, mask=mask, episode=self.episode_count)]

    def _planes(self):
        """The blocks `wedm_normalize` reads, as they lie: the environment's observation and the wire profile's rows."""
        obs = self.env.state.obs
        if self.wire_profile_bins is None:
            return [obs]
        return [obs, self.env.wire_profile(self.wire_profile_bins)["rows"]]

    @staticmethod
    def _raw(obs: torch.Tensor, planes) -> torch.Tensor:
        """`_observation` from the planes already at hand (no second profile launch)."""
        return obs.clone() if len(planes) == 1 else torch.cat([obs, planes[1].t()], dim=1)

    def _observation(self, obs: torch.Tensor) -> torch.Tensor:
        """What `reset` and `step` hand out: a tensor of the caller's own (the environment reuses its block), with the wire
        profile's columns behind the environment's where asked for."""
        if self.wire_profile_bins is None:
            return obs.clone()
        return torch.cat([obs, self.env.wire_profile(self.wire_profile_bins)["rows"].t()], dim=1)

    def _apply_sampler(self, reset_mask: torch.Tensor) -> None:
        if self._geometry_sampler is not None:
            drawn = self._geometry_sampler(self.env, reset_mask)
            self.env.set_geometry(drawn.get("workpiece_height"), drawn.get("wire_diameter_index"), mask=reset_mask, reset=False)
        if self._param_sampler is not None:
            self.env.set_env_params(self._param_sampler(self.env, reset_mask), mask=reset_mask)
        if self._material_sampler is not None:
            self.env.set_wire_material(self._material_sampler(self.env, reset_mask), mask=reset_mask)

    def step(self, action):
        """One control interval for every environment (1000 us by default)."""
        if self._samples and self.autoreset:
            self._apply_sampler(self._need_reset)  # environments about to start a new episode draw their physics
        if self._episode_sampler is not None and self.autoreset:
            self._episode_sampler.draw(self.env, mask=self._need_reset, reset=False)
        if self.autoreset:
            if self._in_kernel_reset:
                # terminated environments are reset by the launch itself; a truncated one is handed to it
                # through its DONE flag (device-side, no synchronisation)
                if self.max_episode_steps is not None:
                    self.env.state.done.logical_or_(self._need_reset)
            elif bool(self._need_reset.any().item()):
                self.env.reset(options={"mask": self._need_reset})  # same key, next episode stream
            self.episode_count += self._need_reset.to(torch.int64)
        # environments this step leaves frozen take no part in the normaliser's statistics or in the episode log
        shaped = self._shaped
        live = None if (self.normalizer is None and self.episode_log is None and shaped is None and self.sensor is None) \
            or self.autoreset else ~self._need_reset
        began = self._need_reset  # who begins an episode in this step: the sensor's `first`
        if shaped is not None:
            shaped.before_launch()
            restarted = self._need_reset if self._in_kernel_reset else None  # whom the launch itself restarts
        prev = {"workpiece_position": self.env.state.workpiece_position.clone()} if self._reward_fn is not None else None
        if prev is not None and self._in_kernel_reset:  # what the kernel's reset will make of the marked environments
            prev["workpiece_position"] = torch.where(self._need_reset, torch.full_like(
                prev["workpiece_position"], float(self.env.config.initial_gap)), prev["workpiece_position"])
        obs, reward, terminated, truncated, info = self.env.step_control(action)
        if shaped is not None:
            reward = shaped.after_launch(restarted, live).clone()
        elif self._reward_fn is not None:
            reward = self._reward_fn(self.env, prev)
        else:
            reward = reward.clone()
        terminated = terminated.clone()
        if self.max_episode_steps is not None:
            truncated = (self.env.state.time >= self.max_episode_steps) & ~terminated
        else:
            truncated = truncated.clone()
        self._need_reset = terminated | truncated
        info = dict(info)  # (StepInfo: the copy composes the exact int64 clock)
        info["episode"] = self.episode_count
        if shaped is not None:
            info["reward_terms"] = shaped.terms
        if self.normalizer is not None:
            norm = self.normalizer
            reward = reward.contiguous()
            planes = self._planes()
            out, scaled = norm.normalize(self._sensed(planes, began, live), reward=reward, terminated=terminated,
                                         truncated=truncated, mask=live)
            info["episode_stats"] = norm.episode_stats
            info["raw_observation"] = self._raw(obs, planes)
            info["raw_reward"] = reward
            if self.episode_log is not None:
                self.episode_log.append(reward, terminated, truncated, mask=live)
            return out, (scaled if norm.reward else reward), terminated, truncated, info
        if self.episode_log is not None:
            reward = reward.contiguous()
            self.episode_log.append(reward, terminated, truncated, mask=live)
        if self.sensor is not None:
            planes = self._planes()
            info["raw_observation"] = self._raw(obs, planes)
            return self._sensed(planes, began, live)[0].t().contiguous(), reward, terminated, truncated, info
        return self._observation(obs), reward, terminated, truncated, info

    def fork(self, src, dst) -> None:
        """`WireEDMEnv.fork`, and the adapter's own per-environment state with it: a destination is due for a reset
        exactly if its source is.  An episode sampler's draw counts stay: a destination keeps its own stream of draws, as
        it keeps its own Philox stream in the physics."""
        from .snapshot import fork_rows

        self.env.fork(src, dst)
        fork_rows(self._need_reset, src, dst)
        if self.normalizer is not None:
            self.normalizer.fork(src, dst)
        if self.episode_log is not None:
            self.episode_log.fork(src, dst)
        if self.sensor is not None:
            self.sensor.fork(src, dst)

    # ---- checkpoints ----
    def _reward_kind(self) -> str:
        if self._shaped is not None:
            return "shaped"
        return "kernel" if self._reward_fn is None else "progress" if self._reward_fn is progress_reward else "callable"

    def _sampler_kinds(self) -> Tuple[str, ...]:
        present = (("param", self._param_sampler), ("material", self._material_sampler), ("geometry", self._geometry_sampler),
                   ("episode", self._episode_sampler))
        return tuple(kind for kind, f in present if f is not None)

    def _settings(self) -> Dict[str, Any]:
        """What changes what a step does, as plain values."""
        out = {"num_envs": self.num_envs, "autoreset": self.autoreset, "max_episode_steps": self.max_episode_steps,
               "wire_profile_bins": self.wire_profile_bins, "obs_names": tuple(self.obs_names), "reward": self._reward_kind(),
               "samplers": self._sampler_kinds()}
        if self._shaped is not None:  # (a ShapedReward keeps nothing across steps: its settings are all there is)
            out.update({f"reward_{key}": value for key, value in self._shaped.settings().items()})
        if self.sensor is not None:  # (the channel set; what the sensor carries across steps is in its own state dict)
            out.update({f"sensor_{key}": value for key, value in self.sensor.settings().items()})
        return out

    def state_dict(self) -> Dict[str, Any]:
        """Everything a bit-identical continuation of the adapter needs: which environments start a new episode at the next
        `step()` (``need_reset``) and their ``episode_count``, the settings that change what a step does (batch size,
        ``autoreset``, ``max_episode_steps``, ``wire_profile_bins``, ``obs_names``, the kind of reward -- ``"kernel"``,
        ``"progress"``, ``"callable"`` or ``"shaped"``, the last with the `ShapedReward`'s ``reward_weights``,
        ``reward_gap_floor`` and ``reward_tmax_ceiling`` -- and the kinds of samplers present), and under ``"env"``, ``"episode_sampler"`` and
        ``"normalizer"``, ``"episode_log"`` and ``"sensor"`` the state dicts of what the adapter owns, each only where it has one.  CPU tensors, ints, strings,
        tuples and lists only: loads with ``weights_only=True``.
        Not in it: ``param_sampler`` / ``material_sampler`` / ``geometry_sampler`` draw from a ``torch.Generator`` the caller
        owns, and a callable reward may hold state of its own -- the caller saves those (``generator.get_state()``)."""
        sd = dict(self._settings())
        sd["need_reset"] = self._need_reset.detach().cpu().clone()
        sd["episode_count"] = self.episode_count.detach().cpu().clone()
        sd["env"] = self.env.state_dict()
        if self._episode_sampler is not None:
            sd["episode_sampler"] = self._episode_sampler.state_dict()
        if self.normalizer is not None:
            sd["normalizer"] = self.normalizer.state_dict()
        if self.episode_log is not None:
            sd["episode_log"] = self.episode_log.state_dict()
        if self.sensor is not None:
            sd["sensor"] = self.sensor.state_dict()
        return sd

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Takes over a `state_dict`.  A dict taken with another batch size, autoreset mode, ``max_episode_steps``, profile
        bins, observation columns or kind of reward, or with a sampler or a normaliser on one side only, raises
        ``ValueError`` naming the difference before anything is written; the nested dicts keep their own refusals (the
        environment's, the episode sampler's spec and batch, the normaliser's columns and batch), all of them checked
        before the first byte changes."""
        mine = self._settings()
        for key, here in mine.items():
            if key not in sd:
                raise ValueError(f"the state dict holds no {key!r}: it is not a WireEDMVectorEnv's")
            there = sd[key]
            if isinstance(here, tuple):
                there = tuple(there)
            if there != here:
                raise ValueError(f"the checkpoint was taken with {key}={sd[key]!r}, this adapter has {key}={here!r}")
        for key, mine_has in (("episode_sampler", self._episode_sampler is not None), ("normalizer", self.normalizer is not None),
                              ("episode_log", self.episode_log is not None), ("sensor", self.sensor is not None)):
            if (key in sd) != mine_has:
                raise ValueError(f"the checkpoint was taken {'with' if key in sd else 'without'} a {key}, this adapter has "
                                 f"{'one' if mine_has else 'none'}")
        for key, shape_of in (("need_reset", self._need_reset), ("episode_count", self.episode_count)):
            if tuple(sd[key].shape) != tuple(shape_of.shape):
                raise ValueError(f"checkpoint tensor {key!r} has shape {tuple(sd[key].shape)}, expected {tuple(shape_of.shape)}")
        s, norm = self._episode_sampler, self.normalizer
        if s is not None:
            ssd = sd["episode_sampler"]
            if ssd["fingerprint"] != s.fingerprint():
                raise ValueError("the checkpoint's EpisodeSampler draws other names or from other ranges than this one")
            if ssd["draw_count"] is not None and tuple(ssd["draw_count"].shape) != (self.num_envs,):
                raise ValueError(f"the checkpoint's draw counts are for {ssd['draw_count'].shape[0]} environments, this "
                                 f"sampler's environment has {self.num_envs}")
        if norm is not None:
            nsd = sd["normalizer"]
            if tuple(nsd["columns"]) != norm.columns:
                raise ValueError(f"the state dict normalises the columns {tuple(nsd['columns'])}, this Normalizer {norm.columns}")
            if int(nsd["num_envs"]) != norm.num_envs:
                raise ValueError(f"the state dict holds {nsd['num_envs']} environments, this Normalizer {norm.num_envs}")
        if self.episode_log is not None:
            self.episode_log.check_state_dict(sd["episode_log"])
        if self.sensor is not None:
            self.sensor.check_state_dict(sd["sensor"])
        self.env.load_state_dict(sd["env"])  # (raises before it writes)
        if s is not None:
            s.load_state_dict(sd["episode_sampler"])
        if norm is not None:
            norm.load_state_dict(sd["normalizer"])
        if self.episode_log is not None:
            self.episode_log.load_state_dict(sd["episode_log"])
        if self.sensor is not None:
            self.sensor.load_state_dict(sd["sensor"])
        self._need_reset = sd["need_reset"].to(device=self.env.device, dtype=torch.bool).clone()
        self.episode_count.copy_(sd["episode_count"])

    def save_checkpoint(self, path) -> None:
        torch.save(self.state_dict(), path)

    def load_checkpoint(self, path) -> None:
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))

    def close(self) -> None:
        self.env.close()
