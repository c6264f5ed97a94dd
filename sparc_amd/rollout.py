"""Rollout storage with GAE advantages and returns computed on the device.

What an on-policy trainer (PPO, A2C) does after ``T`` control steps of a `WireEDMVectorEnv`: rewards and value estimates
become advantages, returns, the mask of the steps that count and the advantages standardised over the rollout, by
`wedm_gae` (include/wedm_hip.h, which holds the definition) in at most three launches without a host synchronisation and
without temporaries.  Two things are the adapter's own: under next-step autoreset the step after a ``terminated`` /
``truncated`` one pairs an observation of the finished episode with a reward of the next and is left out (its stored value
is what the truncated step before it bootstraps from), and the advantage statistics are a fixed pairwise tree over the
global environment index, so they carry the same bits at every launch shape, batch split and after a checkpoint.

`torch_gae` is that definition on host data in NumPy float64: the path of backends without the call (the CPU oracle
backends of the tests) and what the kernels are checked against, bit for bit.  `RolloutBuffer` owns the blocks.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import _abi
from .normalize import TILE, _host, fold, tree

SKIP_AFTER_DONE, NORMALIZE, SCAN, APPLY = _abi.GAE_SKIP_AFTER_DONE, _abi.GAE_NORMALIZE, _abi.GAE_SCAN, _abi.GAE_APPLY
SCAN_UNROLL = 8  # WEDM_GAE_UNROLL of sparc_amd/csrc/wedm_gae.h: steps of the scan kernel's time loop loaded together


def torch_gae(reward, value, last_value, terminated, truncated, *, num_envs: Optional[int] = None, prev_done=None,
              partials=None, tile_offset: int = 0, n_tiles_total: Optional[int] = None, gamma: float = 0.99,
              gae_lambda: float = 0.95, eps: float = 1e-8, flags: int = SKIP_AFTER_DONE | NORMALIZE, advantage=None,
              valid=None) -> Dict[str, torch.Tensor]:
    """The definition of `wedm_gae` on host data.  ``reward`` / ``value``: float32 ``[T, stride]`` blocks (tensors on any
    device or arrays) whose columns ``[0, num_envs)`` are read (default: all); ``terminated`` / ``truncated``: bool or uint8
    of the same shape; ``last_value``: float32 ``[num_envs]``; ``prev_done``: ``[num_envs]`` or None (zeros); ``partials``:
    the ``[n_tiles_total, 3]`` workspace (default: one of exactly this batch's tiles, zeroed); ``advantage`` / ``valid``: what
    an earlier ``SCAN`` left, for a call with ``APPLY`` alone.  Nothing that is passed in is modified.  Returns CPU tensors
    ``[T, num_envs]``: after ``SCAN`` ``advantage``, ``returns``, ``valid`` (uint8), ``prev_done_out`` and ``partials`` (the
    workspace); after ``APPLY`` with ``NORMALIZE`` ``moments`` ``[3]`` and ``advantage_norm``."""
    r = _host(reward)
    N = r.shape[1] if num_envs is None else int(num_envs)
    T = r.shape[0]
    v, te, tr = _host(value), _host(terminated), _host(truncated)
    assert r.dtype == np.float32 and v.dtype == np.float32 and all(a.ndim == 2 and a.shape[0] == T and a.shape[1] >= N
                                                                   for a in (r, v, te, tr))
    if not (N >= 1 and 1 <= T <= _abi.GAE_MAX_STEPS):
        raise ValueError(f"gae: {N} environments x {T} steps, outside [1, ...) x [1, {_abi.GAE_MAX_STEPS}]")
    r, v, te, tr = r[:, :N], v[:, :N], te[:, :N].astype(bool), tr[:, :N].astype(bool)
    normalize = bool(flags & NORMALIZE)
    do_scan = bool(flags & SCAN) or not flags & (SCAN | APPLY)
    do_apply = (bool(flags & APPLY) or not flags & (SCAN | APPLY)) and normalize
    tiles = -(-N // TILE)
    n_tiles_total = tile_offset + tiles if n_tiles_total is None else int(n_tiles_total)
    if not (tile_offset >= 0 and tile_offset + tiles <= n_tiles_total <= _abi.NORM_MAX_TILES):
        raise ValueError("gae: tile range outside the workspace")
    parts = np.zeros((n_tiles_total, _abi.NORM_MOMENTS), dtype=np.float64) if partials is None else \
        _host(partials, np.float64).copy()
    assert parts.shape == (n_tiles_total, _abi.NORM_MOMENTS)
    out: Dict[str, Any] = {}

    if do_scan:
        gamma64 = np.float64(gamma)
        gl = gamma64 * np.float64(gae_lambda)
        done = te | tr
        prev = np.zeros(N, dtype=bool) if prev_done is None else _host(prev_done).reshape(-1)[:N].astype(bool)
        skip = np.concatenate([prev[None], done[:-1]]) if flags & SKIP_AFTER_DONE else np.zeros((T, N), dtype=bool)
        adv, ret = np.empty((T, N), dtype=np.float32), np.empty((T, N), dtype=np.float32)
        A = np.zeros(N, dtype=np.float64)
        nv = _host(last_value).reshape(-1)[:N].astype(np.float64)
        n, m, S = (np.zeros(tiles * TILE, dtype=np.float64) for _ in range(3))
        with np.errstate(all="ignore"):
            for t in range(T - 1, -1, -1):
                val = v[t].astype(np.float64)
                delta = (r[t].astype(np.float64) + np.where(te[t], 0.0, gamma64 * nv)) - val
                A = np.where(skip[t], 0.0, delta + np.where(done[t], 0.0, gl * A))
                adv[t] = A.astype(np.float32)
                ret[t] = (A + val).astype(np.float32)
                nv = val
                if normalize:
                    x = adv[t].astype(np.float64)
                    n1 = n[:N] + 1.0
                    d = x - m[:N]
                    m1 = m[:N] + d / n1
                    S1 = S[:N] + d * (x - m1)
                    take = ~skip[t]
                    n[:N], m[:N], S[:N] = np.where(take, n1, n[:N]), np.where(take, m1, m[:N]), np.where(take, S1, S[:N])
        if normalize:  # the tile's eight levels over the environments' triples, EMPTY past the batch's end
            node = tree(*(a.reshape(tiles, TILE).T for a in (n, m, S)))
            parts[tile_offset: tile_offset + tiles] = np.stack(node, axis=1)
        out.update(advantage=torch.from_numpy(adv), returns=torch.from_numpy(ret),
                   valid=torch.from_numpy((~skip).astype(np.uint8)), prev_done_out=torch.from_numpy(done[T - 1].astype(np.uint8)))
    out["partials"] = torch.from_numpy(parts)

    if do_apply:
        adv = out["advantage"].numpy() if do_scan else _host(advantage)[:, :N]
        ok = (out["valid"].numpy() if do_scan else _host(valid)[:, :N]).astype(bool)
        assert adv.dtype == np.float32 and adv.shape == (T, N) and ok.shape == (T, N)
        n, m, S = fold(parts.reshape(n_tiles_total, _abi.NORM_MOMENTS, 1))[:, 0]
        with np.errstate(all="ignore"):
            y = ((adv.astype(np.float64) - m) / np.sqrt(S / n + np.float64(eps))).astype(np.float32)
        out["moments"] = torch.from_numpy(np.array([n, m, S], dtype=np.float64))
        out["advantage_norm"] = torch.from_numpy(np.where(ok & (n != 0.0), y, np.float32(0.0)))
    return out


def device_gae(desc: "_abi.GaeDesc", device) -> None:
    """`wedm_gae` on ``device`` and torch's current stream, for callers that hold no environment."""
    from . import _lib

    _lib.call_stateless(_lib.load().wedm_gae, torch.device(device), C.byref(desc))


def _leaves(action, path: str = "action") -> List[Tuple[str, torch.Tensor]]:
    """An action's tensors by key path: a tensor, a (nested) dict of tensors, or a `DeviceAction`."""
    if torch.is_tensor(action):
        return [(path, action)]
    if isinstance(action, dict):
        return [leaf for k, v in action.items() for leaf in _leaves(v, f"{path}.{k}")]
    slots = getattr(type(action), "__slots__", ())
    found = [(f"{path}.{k}", getattr(action, k)) for k in slots if torch.is_tensor(getattr(action, k, None))]
    if not found:
        raise ValueError(f"add: an action is a tensor, a dict of tensors or a DeviceAction, not {type(action).__name__}")
    return found


class RolloutBuffer:
    """``num_steps`` control steps of a `WireEDMVectorEnv`'s transitions on its device, and what `wedm_gae` makes of them.

    ``gamma`` / ``gae_lambda``: discount and GAE's lambda.  ``normalize_advantage``: also standardise the advantages over
    the rollout's valid steps (``advantage_norm``; ``eps`` is added to the variance before its root).  ``skip_after_done``:
    leave out the step after a done one, which under the adapter's next-step autoreset pairs the finished episode's final
    observation with the next episode's reward (``valid`` is 0 there, its advantage 0, its return its value).  ``extras``:
    further per-step blocks by name and dtype, such as ``{"log_prob": torch.float32}``.

    Per control step: ``add(obs, action, value, reward, terminated, truncated)`` with the observation the action was chosen
    from and what ``vec.step(action)`` returned for it; after ``num_steps`` of them ``finish(last_value)`` with the value
    estimate at the observation the last step returned.  The blocks of the action's leaves are allocated by the first
    `add`, from its tensors' dtypes and shapes; everything else by the constructor."""

    def __init__(self, vec, num_steps: int, *, gamma: float = 0.99, gae_lambda: float = 0.95, normalize_advantage: bool = True,
                 eps: float = 1e-8, skip_after_done: bool = True, extras: Optional[Dict[str, torch.dtype]] = None):
        T, N = int(num_steps), int(vec.num_envs)
        if not 1 <= T <= _abi.GAE_MAX_STEPS:
            raise ValueError(f"num_steps must lie in [1, {_abi.GAE_MAX_STEPS}], got {num_steps}")
        if not all(np.isfinite(x) for x in (gamma, gae_lambda, eps)):
            raise ValueError("gamma, gae_lambda and eps must be finite")
        self.num_steps, self.num_envs, self.device = T, N, torch.device(vec.env.device)
        self.gamma, self.gae_lambda, self.eps = float(gamma), float(gae_lambda), float(eps)
        self.normalize_advantage, self.skip_after_done = bool(normalize_advantage), bool(skip_after_done)
        backend = getattr(vec.env, "_backend", None)
        self._native = backend if hasattr(backend, "gae") else None
        self._tiles = -(-N // TILE)
        if self._tiles > _abi.NORM_MAX_TILES:
            raise ValueError(f"a RolloutBuffer serves at most {_abi.NORM_MAX_TILES * TILE} environments")
        kw = dict(device=self.device)
        block = lambda dtype, *rest: torch.zeros((T, N) + rest, dtype=dtype, **kw)
        self.stored: Dict[str, torch.Tensor] = {
            "obs": block(torch.float32, len(vec.obs_names)), "value": block(torch.float32), "reward": block(torch.float32),
            "terminated": block(torch.bool), "truncated": block(torch.bool)}
        self.extras = dict(extras or {})
        for name, dtype in self.extras.items():
            if name in self.stored or name.startswith("action"):
                raise ValueError(f"extras: the name {name!r} is taken")
            self.stored[name] = block(dtype)
        self._action_keys: Optional[Tuple[str, ...]] = None
        self.computed: Dict[str, torch.Tensor] = {"advantage": block(torch.float32), "returns": block(torch.float32),
                                                  "valid": block(torch.uint8)}
        if self.normalize_advantage:
            self.computed["advantage_norm"] = block(torch.float32)
        self._prev_done = torch.zeros(N, dtype=torch.uint8, **kw)
        self._partials = torch.zeros((self._tiles, _abi.NORM_MOMENTS), dtype=torch.float64, **kw)
        self.moments = torch.zeros(_abi.NORM_MOMENTS, dtype=torch.float64, **kw)
        self._slot = 0
        self._finished = False  # `finish` has run and no `add` since: the computed blocks belong to the stored steps
        self._keep = None
        s, c = self.stored, self.computed
        self._desc = _abi.GaeDesc(
            reward=s["reward"].data_ptr(), value=s["value"].data_ptr(), terminated=s["terminated"].data_ptr(),
            truncated=s["truncated"].data_ptr(), prev_done_in=self._prev_done.data_ptr(), advantage=c["advantage"].data_ptr(),
            returns=c["returns"].data_ptr(), valid=c["valid"].data_ptr(), prev_done_out=self._prev_done.data_ptr(),
            advantage_norm=c["advantage_norm"].data_ptr() if self.normalize_advantage else None,
            partials=self._partials.data_ptr(), moments=self.moments.data_ptr(), in_stride=N, out_stride=N, T=T, num_envs=N,
            tile_offset=0, n_tiles_total=self._tiles)
        self._settings_to_desc()

    def _settings_to_desc(self) -> None:
        d = self._desc
        d.gamma, d.lam, d.eps = self.gamma, self.gae_lambda, self.eps
        d.flags = (SKIP_AFTER_DONE if self.skip_after_done else 0) | (NORMALIZE if self.normalize_advantage else 0)

    # ------------------------------------------------------------------ storing
    def _check(self, name: str, t, shape: Tuple[int, ...], dtype: torch.dtype) -> None:
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.device.type != self.device.type or (self.device.index is not None and t.device.index != self.device.index):
            raise ValueError(f"{name} lies on {t.device}, the buffer on {self.device}")
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}")

    def add(self, obs, action, value, reward, terminated, truncated, **extras) -> None:
        """One control step into the next slot: ``obs`` the observation the action was chosen from, ``value`` the estimate at
        it, ``reward`` / ``terminated`` / ``truncated`` what ``step(action)`` returned.  Copies only: no allocation (after
        the first call) and no host synchronisation."""
        t, N, s = self._slot, self.num_envs, self.stored
        if t >= self.num_steps:
            raise ValueError(f"add: the buffer holds {self.num_steps} steps; call finish()")
        if set(extras) != set(self.extras):
            raise ValueError(f"add: extras {sorted(extras)} given, {sorted(self.extras)} expected")
        leaves = _leaves(action)
        if self._action_keys is None:
            for key, leaf in leaves:
                self._check(key, leaf, (N,) + tuple(leaf.shape[1:]), leaf.dtype)
                s[key] = torch.zeros((self.num_steps,) + tuple(leaf.shape), dtype=leaf.dtype, device=self.device)
            self._action_keys = tuple(key for key, _ in leaves)
        if tuple(key for key, _ in leaves) != self._action_keys:
            raise ValueError(f"add: the action's leaves are {[k for k, _ in leaves]}, the first add's {list(self._action_keys)}")
        given = dict(leaves, obs=obs, value=value, reward=reward, terminated=terminated, truncated=truncated, **extras)
        for name, x in given.items():
            self._check(name, x, tuple(s[name].shape[1:]), s[name].dtype)
        for name, x in given.items():
            s[name][t].copy_(x)
        self._slot = t + 1
        self._finished = False

    # ------------------------------------------------------------------ the call
    def finish(self, last_value: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One `wedm_gae` call over the stored steps; ``last_value``: float32 ``[num_envs]``, the estimate at the observation
        the last step returned.  Returns the ``[T, N]`` tensors ``advantage``, ``returns``, ``valid`` (bool) and, with
        ``normalize_advantage``, ``advantage_norm`` (`moments` holds their count, mean and sum of squared deviations): the
        buffer's own blocks, valid until the next `finish`.  The last step's done row becomes the next rollout's
        ``prev_done`` and the buffer starts again at slot 0."""
        if self._slot != self.num_steps:
            raise ValueError(f"finish: {self._slot} of {self.num_steps} steps are stored")
        self._check("last_value", last_value, (self.num_envs,), torch.float32)
        s, c = self.stored, self.computed
        if self._native is None:
            d = self._desc
            out = torch_gae(s["reward"], s["value"], last_value, s["terminated"], s["truncated"], prev_done=self._prev_done,
                            gamma=self.gamma, gae_lambda=self.gae_lambda, eps=self.eps, flags=d.flags)
            for name, t in c.items():
                t.copy_(out[name])
            self._prev_done.copy_(out["prev_done_out"])
            if self.normalize_advantage:
                self._partials.copy_(out["partials"])
                self.moments.copy_(out["moments"])
        else:
            last_value = last_value.contiguous()
            self._desc.last_value = last_value.data_ptr()
            self._native.gae(self._desc)
            self._keep = last_value  # the launches are asynchronous: their input lives until the next call
        self._slot = 0
        self._finished = True
        return self._results()

    def _results(self) -> Dict[str, torch.Tensor]:
        return {k: (v.view(torch.bool) if k == "valid" else v) for k, v in self.computed.items()}

    def flat(self) -> Dict[str, torch.Tensor]:
        """Every stored and computed block as a ``[T * N, ...]`` view (no copy), step-major."""
        TN = self.num_steps * self.num_envs
        return {k: v.view((TN,) + tuple(v.shape[2:])) for k, v in {**self.stored, **self._results()}.items()}

    def minibatches(self, n: int, generator: Optional[torch.Generator] = None, sampler=None) -> Iterator[Dict[str, torch.Tensor]]:
        """``n`` disjoint index-selected parts of `flat` that together cover the rollout, in the order of a device
        ``randperm`` (``generator`` must live on the buffer's device when given).  Skipped steps are among them: weigh the
        loss by ``valid``.  With ``sampler``, a `MinibatchSampler` of this buffer with ``n`` parts, the parts are those of
        its next `draw` instead: a seeded permutation a checkpoint carries, the valid steps spread evenly and first in
        every part."""
        flat = self.flat()
        if sampler is not None:
            if sampler.buf is not self or int(n) != sampler.n_parts or generator is not None:
                raise ValueError(f"minibatches: the sampler must be this buffer's, n ({n}) its n_parts ({sampler.n_parts}), and "
                                 "no generator given")
            parts = sampler.draw()
        else:
            perm = torch.randperm(self.num_steps * self.num_envs, device=self.device, generator=generator)
            parts = torch.tensor_split(perm, int(n))
        for idx in parts:
            yield {k: v[idx] for k, v in flat.items()}

    def reset(self) -> None:
        """Forgets the stored steps and the last done row: call it after ``vec.reset()``."""
        self._prev_done.zero_()
        self._slot = 0
        self._finished = False

    @property
    def prev_done(self) -> torch.Tensor:
        """uint8 ``[N]``: whether the step before slot 0 was a done one (the buffer's live row)."""
        return self._prev_done

    # ------------------------------------------------------------------ checkpoints
    def settings(self) -> Dict[str, Any]:
        return dict(gamma=self.gamma, gae_lambda=self.gae_lambda, eps=self.eps, normalize_advantage=self.normalize_advantage,
                    skip_after_done=self.skip_after_done)

    def state_dict(self) -> Dict[str, Any]:
        """The settings, the slot, ``prev_done`` and the steps stored so far, as CPU tensors and plain values.  Between `finish`
        and the next `add` -- where the epochs over the rollout run -- the rollout is whole: every stored step, and under
        ``"computed"`` what `finish` made of them (``moments`` included), so that `flat` and `minibatches` go on after a load."""
        rows = self.num_steps if self._finished else self._slot
        sd = {"num_steps": self.num_steps, "num_envs": self.num_envs, "settings": self.settings(), "slot": self._slot,
              "prev_done": self._prev_done.detach().cpu().clone(),
              "stored": {k: v[:rows].detach().cpu().clone() for k, v in self.stored.items()}}
        if self._finished:
            sd["computed"] = {**{k: v.detach().cpu().clone() for k, v in self.computed.items()},
                              "moments": self.moments.detach().cpu().clone()}
        return sd

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Takes over a `state_dict` of a buffer of the same shape, with the same normalisation block and extras."""
        if (int(sd["num_steps"]), int(sd["num_envs"])) != (self.num_steps, self.num_envs):
            raise ValueError(f"the state dict holds {sd['num_steps']} steps x {sd['num_envs']} environments, this buffer "
                             f"{self.num_steps} x {self.num_envs}")
        st = sd["settings"]
        if bool(st["normalize_advantage"]) != self.normalize_advantage:
            raise ValueError("the state dict's normalize_advantage differs from this buffer's")
        stored = sd["stored"]
        actions = tuple(k for k in stored if k.startswith("action"))
        if {k for k in stored if k not in actions} != {k for k in self.stored if not k.startswith("action")}:
            raise ValueError(f"the state dict stores {sorted(stored)}, this buffer {sorted(self.stored)}")
        if self._action_keys is not None and actions and actions != self._action_keys:
            raise ValueError(f"the state dict's action leaves are {list(actions)}, this buffer's {list(self._action_keys)}")
        self.gamma, self.gae_lambda, self.eps = float(st["gamma"]), float(st["gae_lambda"]), float(st["eps"])
        self.skip_after_done = bool(st["skip_after_done"])
        self._settings_to_desc()
        slot = int(sd["slot"])
        computed = sd.get("computed")  # the whole rollout of a dict taken between `finish` and the next `add`
        rows = self.num_steps if computed is not None else slot
        if self._action_keys is None and rows > 0:
            for k in actions:
                self.stored[k] = torch.zeros((self.num_steps,) + tuple(stored[k].shape[1:]), dtype=stored[k].dtype, device=self.device)
            self._action_keys = actions
        for k, v in stored.items():
            if rows > 0:
                self.stored[k][:rows].copy_(v)
        if computed is not None:
            for k, t in self.computed.items():
                t.copy_(computed[k])
            self.moments.copy_(computed["moments"])
        self._prev_done.copy_(torch.as_tensor(sd["prev_done"]).to(torch.uint8))
        self._slot = slot
        self._finished = computed is not None
