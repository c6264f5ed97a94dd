"""Adam with global-norm gradient clipping and a KL gate on the device, one call per minibatch.

The step from ``theta.grad`` to the next ``theta``: what ``torch.nn.utils.clip_grad_norm_``, ``torch.optim.AdamW`` and a host
``if approx_kl > limit: break`` compose is one call of `wedm_adam` (include/wedm_hip.h, which holds the definition with
every rounding).  The gradient's norm is a fixed pairwise tree over the element number, Adam's moments and bias-correction
products are blocks a checkpoint carries, and the KL early stop is a latch on the device: the host never reads a value.

`adam_reference` is that definition on host data in NumPy float64: the path of CPU devices (the oracle-backend stacks of the
tests) and what the kernels are checked against, bit for bit.  `Adam` owns the moments, the state and the workspace.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _abi
from .policy_head import _f32
from .ppo import _f64, pairwise_sum

TILE = _abi.NORM_TILE
MAX_N = _abi.NORM_MAX_TILES * TILE  # entries of a parameter block at most: 1 048 576
ONE_BLOCK_MAX = _abi.OPT_ONE_BLOCK_MAX
STATE_NAMES, INFO_NAMES = _abi.OPT_STATE_NAMES, _abi.OPT_INFO_NAMES
B1POW, B2POW, T, SKIPPED_NONFINITE, SKIPPED_KL, LATCH = range(6)  # enum wedm_opt_state
SUMSQ, NORM, SCALE, LR, APPLIED, KL, BC1, BC2 = range(8)  # enum wedm_opt_info
FRESH_STATE = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def check_scalars(lr, betas, eps, weight_decay, max_norm, kl_limit) -> Tuple[float, ...]:
    """The descriptor's scalars as floats, or ValueError with the header's conditions."""
    lr, (beta1, beta2), eps, weight_decay = float(lr), (float(b) for b in betas), float(eps), float(weight_decay)
    if not math.isfinite(lr) or lr < 0.0:
        raise ValueError(f"adam: lr must be finite and not negative, got {lr}")
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError(f"adam: betas must lie in [0, 1), got {(beta1, beta2)}")
    if not math.isfinite(eps) or not eps > 0.0:
        raise ValueError(f"adam: eps must be finite and positive, got {eps}")
    if not math.isfinite(weight_decay) or weight_decay < 0.0:
        raise ValueError(f"adam: weight_decay must be finite and not negative, got {weight_decay}")
    if max_norm is not None and (not math.isfinite(float(max_norm)) or not float(max_norm) > 0.0):
        raise ValueError(f"adam: max_norm must be finite and positive, got {max_norm}")
    if kl_limit is not None and (not math.isfinite(float(kl_limit)) or float(kl_limit) < 0.0):
        raise ValueError(f"adam: kl_limit must be finite and not negative, got {kl_limit}")
    return lr, beta1, beta2, eps, weight_decay, None if max_norm is None else float(max_norm), None if kl_limit is None else float(kl_limit)


def adam_reference(theta: np.ndarray, m: np.ndarray, v: np.ndarray, grad: np.ndarray, state: np.ndarray, *, lr: float,
                   betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-5, weight_decay: float = 0.0,
                   max_norm: Optional[float] = None, kl: Optional[float] = None, kl_limit: Optional[float] = None,
                   new_update: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of `wedm_adam` (include/wedm_hip.h) on host data, NumPy float64 with the header's roundings, IN PLACE.

    ``theta``, ``m``, ``v``: float32 ``[n]``, written only when the call is applied; ``grad``: float32 ``[n]``, read;
    ``state``: float64 ``[8]`` (`STATE_NAMES`, then two zeros), read and written.  ``max_norm`` None: no clipping;
    ``kl_limit`` None: no gate, and ``kl`` (one float64, a NaN allowed) is not looked at.  Returns ``info`` (float64 ``[8]``:
    `INFO_NAMES`) and ``partials`` (float64 ``[ceil(n / 256)]``: the tiles' nodes of the tree of the squared gradient)."""
    lr, beta1, beta2, eps, weight_decay, max_norm, kl_limit = check_scalars(lr, betas, eps, weight_decay, max_norm, kl_limit)
    for name, a in (("theta", theta), ("m", m), ("v", v), ("grad", grad)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 1 or a.shape != theta.shape:
            raise ValueError(f"adam: {name} must be a float32 array [n] like theta")
    n = theta.shape[0]
    if n < 1 or n > MAX_N:
        raise ValueError(f"adam: a parameter block holds 1 to {MAX_N} entries, got {n}")
    if not isinstance(state, np.ndarray) or state.dtype != np.float64 or state.shape != (_abi.OPT_STATE,):
        raise ValueError(f"adam: state must be a float64 array [{_abi.OPT_STATE}]")
    if kl_limit is not None and kl is None:
        raise ValueError("adam: kl_limit is set: kl is needed")
    f64 = np.float64
    with np.errstate(all="ignore"):
        g64 = grad.astype(f64)
        partials, S = pairwise_sum(g64 * g64)
        S = f64(S)
        latch = f64(0.0) if new_update else f64(state[LATCH])
        klv = f64(np.asarray(kl, dtype=f64).reshape(-1)[0]) if kl_limit is not None else f64(0.0)
        if kl_limit is not None and latch == 0.0 and not klv <= kl_limit:
            latch = f64(1.0)
        finite = bool(S < np.inf)
        norm = np.sqrt(S)
        c = f64(1.0)
        if max_norm is not None:
            c = f64(max_norm) / (norm + f64(1e-6))
            if not c < 1.0:
                c = f64(1.0)
        if latch != 0.0:
            state[SKIPPED_KL] += 1.0
        elif not finite:
            state[SKIPPED_NONFINITE] += 1.0
        else:
            state[T] += 1.0
            state[B1POW] = state[B1POW] * f64(beta1)
            state[B2POW] = state[B2POW] * f64(beta2)
        applied = latch == 0.0 and finite
        bc1, bc2 = f64(1.0) - state[B1POW], f64(1.0) - state[B2POW]
        state[LATCH] = latch
        state[6:] = 0.0
        state[:] = _f64(state)
        info = _f64(np.array([S, norm, c, lr, 1.0 if applied else 0.0, klv, bc1, bc2], dtype=f64))
        if applied:
            g = g64 * c
            p = theta.astype(f64)
            if weight_decay != 0.0:
                p = p - (f64(lr) * f64(weight_decay)) * p
            mf = _f32(f64(beta1) * m.astype(f64) + (f64(1.0) - f64(beta1)) * g)
            vf = _f32(f64(beta2) * v.astype(f64) + (f64(1.0) - f64(beta2)) * (g * g))
            mh, vh = mf.astype(f64) / bc1, vf.astype(f64) / bc2
            p = p - f64(lr) * (mh / (np.sqrt(vh) + f64(eps)))
            theta[:], m[:], v[:] = _f32(p), mf, vf
    return info, _f64(partials)


def device_adam(desc: "_abi.OptDesc", device) -> None:
    """`wedm_adam` on ``device`` and torch's current stream, for callers that hold no environment."""
    from . import _lib

    _lib.call_stateless(_lib.load().wedm_adam, torch.device(device), C.byref(desc))


class Adam:
    """``Adam(target, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.0, max_grad_norm=None, kl_limit=None)``: Adam (AdamW
    with ``weight_decay``) over one flat parameter block, with global-norm gradient clipping (``max_grad_norm``) and an early
    stop on PPO's approximate KL (``kl_limit``), as one `wedm_adam` per minibatch.

    ``target`` is a `PolicyNet` (its ``theta``) or one flat contiguous float32 leaf.  ``lr`` is a float or a callable of the
    call number (0, 1, ...; skipped calls count), evaluated on the host: a schedule depends on nothing the device knows.
    The moments ``m``, ``v``, the ``state`` (`STATE_NAMES`), ``info`` (`INFO_NAMES`, of the last call) and the tree's workspace
    are allocated here, once; `step` allocates nothing and never synchronises with the host.  A minibatch whose gradient holds
    a NaN or an infinity is skipped and counted; with ``kl_limit``, a minibatch whose ``approx_kl`` exceeds it (or is a NaN)
    is skipped together with every later one until `begin_update`.  On a CPU device every call runs `adam_reference`."""

    def __init__(self, target, lr: Union[float, Callable[[int], float]] = 3e-4, betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-5,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, kl_limit: Optional[float] = None):
        theta = getattr(target, "theta", target)
        if not torch.is_tensor(theta) or theta.dtype != torch.float32 or theta.ndim != 1 or not theta.is_contiguous() \
                or not theta.is_leaf or not theta.requires_grad:
            raise ValueError("Adam: the target must be a PolicyNet or one flat contiguous float32 leaf that requires a gradient")
        if not 1 <= theta.shape[0] <= MAX_N:
            raise ValueError(f"Adam: a parameter block holds 1 to {MAX_N} entries, got {theta.shape[0]}")
        self.theta, self.device, self.n = theta, theta.device, int(theta.shape[0])
        self._set(lr, betas, eps, weight_decay, max_grad_norm, kl_limit)
        self._native = None
        if self.device.type == "cuda":
            native = getattr(target, "_native", None)
            self._native = native.adam if hasattr(native, "adam") else (lambda d: device_adam(d, self.device))
        kw = dict(device=self.device)
        self.m = torch.zeros(self.n, dtype=torch.float32, **kw)
        self.v = torch.zeros(self.n, dtype=torch.float32, **kw)
        self.state = torch.tensor(FRESH_STATE, dtype=torch.float64, **kw)
        self._info = torch.zeros(_abi.OPT_INFO, dtype=torch.float64, **kw)
        self._partials = torch.zeros(-(-self.n // TILE), dtype=torch.float64, **kw)
        self.calls, self._new_update = 0, False
        self._keep = None  # the inputs of the launches in flight

    def _set(self, lr, betas, eps, weight_decay, max_grad_norm, kl_limit) -> None:
        fixed = 0.0 if callable(lr) else lr
        _, b1, b2, eps, wd, max_norm, kl_limit = check_scalars(fixed, betas, eps, weight_decay, max_grad_norm, kl_limit)
        self.lr = lr if callable(lr) else float(lr)
        self.betas, self.eps, self.weight_decay, self.max_grad_norm, self.kl_limit = (b1, b2), eps, wd, max_norm, kl_limit

    # ------------------------------------------------------------------ the call
    def begin_update(self) -> None:
        """The next `step` opens the KL gate again (it carries WEDM_OPT_NEW_UPDATE): call it once per rollout, before the
        first minibatch of its epochs.  Launches nothing."""
        self._new_update = True

    def zero_grad(self) -> None:
        """``theta.grad = None``: a `PolicyNet` then writes its own gradient buffer without adding to it."""
        self.theta.grad = None

    def _kl(self, stats) -> Optional[torch.Tensor]:
        if self.kl_limit is None:
            return None
        t = getattr(stats, "tensor", stats)
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != (_abi.PPO_STATS,) or not t.is_contiguous() \
                or t.device != self.device:
            raise ValueError("Adam.step: kl_limit is set: stats must be what PPOLoss.backward returned (or its float64 [8] tensor) "
                             "on the parameters' device")
        return t

    def step(self, stats=None) -> None:
        """One `wedm_adam` on torch's current stream: ``theta.grad`` into ``theta``, ``m``, ``v``, ``state`` and ``info``.
        ``stats`` is what ``PPOLoss.backward`` returned -- its device tensor's ``approx_kl`` entry is read by the call, on
        the device --, needed when ``kl_limit`` is set.  Raises if ``theta.grad`` is None."""
        theta, grad = self.theta, self.theta.grad
        if grad is None:
            raise RuntimeError("Adam.step: theta.grad is None: run a backward pass first")
        if grad.dtype != torch.float32 or grad.shape != theta.shape or not grad.is_contiguous() or grad.device != theta.device:
            raise ValueError("Adam.step: theta.grad must be a contiguous float32 tensor like theta")
        stats_t = self._kl(stats)
        lr = float(self.lr(self.calls)) if callable(self.lr) else self.lr
        if not math.isfinite(lr) or lr < 0.0:
            raise ValueError(f"Adam.step: lr must be finite and not negative, got {lr} at call {self.calls}")
        if self._native is not None:
            flags = (_abi.OPT_CLIP if self.max_grad_norm is not None else 0) | (_abi.OPT_KL_GATE if stats_t is not None else 0) \
                | (_abi.OPT_NEW_UPDATE if self._new_update else 0)
            d = _abi.OptDesc(theta=theta.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), grad=grad.data_ptr(),
                             partials=self._partials.data_ptr(), state=self.state.data_ptr(), info=self._info.data_ptr(),
                             kl=None if stats_t is None else stats_t.data_ptr() + 8 * _abi.PPO_STAT_NAMES.index("approx_kl"),
                             lr=lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay,
                             max_norm=0.0 if self.max_grad_norm is None else self.max_grad_norm,
                             kl_limit=0.0 if self.kl_limit is None else self.kl_limit, n=self.n, flags=flags)
            self._native(d)
            self._keep = (grad, stats_t)  # the launches are asynchronous: their inputs live until the next call
        else:
            info, partials = adam_reference(
                theta.detach().numpy(), self.m.numpy(), self.v.numpy(), grad.numpy(), self.state.numpy(), lr=lr, betas=self.betas,
                eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_grad_norm,
                kl=None if stats_t is None else float(stats_t[_abi.PPO_STAT_NAMES.index("approx_kl")]), kl_limit=self.kl_limit,
                new_update=self._new_update)
            self._info.copy_(torch.from_numpy(info))
            self._partials.copy_(torch.from_numpy(partials))
        self.calls += 1
        self._new_update = False

    @property
    def info(self) -> torch.Tensor:
        """The last call's ``[8]`` float64 device tensor (`INFO_NAMES`; indices `SUMSQ` ... `BC2`): the optimiser's own,
        rewritten by its next `step`."""
        return self._info

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        """``m``, ``v``, ``state``, the hyperparameters (``lr`` None where it is a callable, which stays the object's), the
        call number and whether a `begin_update` is pending."""
        return {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(), "state": self.state.detach().cpu().clone(),
                "lr": None if callable(self.lr) else self.lr, "betas": list(self.betas), "eps": self.eps,
                "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm, "kl_limit": self.kl_limit,
                "calls": self.calls, "new_update": self._new_update}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Refuses moments of another length (and then leaves every byte as it was); takes the dict's hyperparameters."""
        for k, dtype, shape in (("m", torch.float32, (self.n,)), ("v", torch.float32, (self.n,)), ("state", torch.float64, (_abi.OPT_STATE,))):
            t = sd[k]
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError(f"Adam: {k} must be a {dtype} tensor {list(shape)}")
        if sd["lr"] is None and not callable(self.lr):
            raise ValueError("Adam: the dict was written with a callable lr, which it does not carry: build this Adam with one")
        self._set(self.lr if sd["lr"] is None else sd["lr"], sd["betas"], sd["eps"], sd["weight_decay"], sd["max_grad_norm"], sd["kl_limit"])
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.state.copy_(sd["state"])
        self.calls, self._new_update = int(sd["calls"]), bool(sd["new_update"])
