"""PPO's clipped loss and its gradient on the device, one call per minibatch.

The last link of the on-policy loop: what `PolicyHead.evaluate`, a dozen torch launches on ``[B]`` tensors and autograd
compose by hand -- ratio, clip, minimum, value loss, entropy bonus, their means over the steps that count, and the gradient
with respect to the policy's parameter rows and the value estimates -- is one call of `wedm_ppo_loss` (include/wedm_hip.h,
which holds the definition with every rounding).  The distribution is evaluated once per row, the means are a fixed pairwise
tree over the row number (so their bits depend on the values and the rows' order alone), ``valid`` is applied by the call,
and the stored blocks of a `RolloutBuffer` can be read in place through an index instead of being gathered per minibatch.

`ppo_loss_definition` is that definition on host data in NumPy float64, built on `policy_head_definition`'s pieces: the path
of backends without the call (the CPU oracle backends of the tests) and what the kernels are checked against, bit for bit.
`PPOLoss` owns the workspace and the gradient buffers.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional, Sequence

import numpy as np
import torch

from . import _abi
from .normalize import _host
from .policy_head import BACKWARD, EVALUATE, PolicyHead, _f32, policy_head_definition, portable_exp

TILE = _abi.NORM_TILE
MAX_ROWS = _abi.NORM_MAX_TILES * TILE  # rows of a minibatch at most: 1 048 576
STAT_NAMES = _abi.PPO_STAT_NAMES
_NAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def _f64(x: np.ndarray) -> np.ndarray:
    """Every float64 the call stores: a NaN becomes 0x7FF8000000000000."""
    return np.where(x != x, _NAN64, x)


def pairwise_sum(leaves: np.ndarray) -> np.ndarray:
    """The definition's tree over axis 0 of ``[rows, ...]`` float64: (tile nodes ``[tiles, ...]``, root).  Rows are padded
    with +0.0 to tiles of 256, a tile's eight levels come first, then the pairwise tree over the tile index, padded with
    +0.0 to the smallest power of two that holds the tiles; the lower index is on the left, additions are plain."""
    x = np.asarray(leaves, dtype=np.float64)
    rows = x.shape[0]
    tiles = -(-rows // TILE)
    with np.errstate(all="ignore"):
        level = np.zeros((tiles * TILE,) + x.shape[1:])
        level[:rows] = x
        for _ in range(8):
            level = level[0::2] + level[1::2]
        nodes = level
        padded = 1
        while padded < tiles:
            padded *= 2
        level = np.zeros((padded,) + x.shape[1:])
        level[:tiles] = nodes
        while level.shape[0] > 1:
            level = level[0::2] + level[1::2]
    return nodes, level[0]


def ppo_loss_definition(params, value, *, modes: Sequence[int], lo, hi, log_span=None, u, mode_index, old_log_prob, advantage,
                        returns, old_value=None, valid=None, index=None, clip: float = 0.2, vf_coef: float = 0.5,
                        ent_coef: float = 0.0, clip_value: Optional[float] = None) -> Dict[str, np.ndarray]:
    """The definition of `wedm_ppo_loss` (include/wedm_hip.h) on host data, NumPy float64 with the header's roundings.

    ``params``: float32 ``[B, >= 8 + M]`` and ``value``: float32 ``[B]``, dense by row.  The stored inputs ``u`` (float32
    ``[n_src, 4]``), ``mode_index`` (int32), ``old_log_prob``, ``advantage``, ``returns``, ``old_value`` (float32; read only
    when ``clip_value`` is given) and ``valid`` (bool / uint8, or None) are read at ``index[r]`` (int64 ``[B]``; None: at
    ``r``, and then ``n_src == B``).  A row whose index lies outside ``[0, n_src)`` is never read, is not live and counts in
    ``n_bad``; a row with ``valid == 0`` is not live.  Returns ``stats`` (float64 ``[8]``: `STAT_NAMES`), ``partials``
    (float64 ``[tiles, 7]``), ``count`` (int32 ``[2]``: live and bad rows), ``grad_params`` (float32 ``[B, 8 + M]``) and
    ``grad_value`` (float32 ``[B]``) -- the gradient of ``stats[2]``, the loss, with the float32 rounding of the
    log-probability taken as the identity --, the unrounded ``grad_params64`` / ``grad_value64``, and the rows' terms
    ``live``, ``ratio``, ``clipped`` (bool) and ``summands`` (float64 ``[B, 7]``, the leaves of the tree) for whoever wants
    to count branches or add them up again.  Nothing that is passed in is modified."""
    p = _host(params)
    M = len(list(modes))
    P = 8 + M
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < P or p.shape[0] < 1:
        raise ValueError(f"ppo loss: params must be float32 [rows >= 1, >= {P}], got {p.dtype} {list(p.shape)}")
    B = p.shape[0]
    if B > MAX_ROWS:
        raise ValueError(f"ppo loss: a minibatch holds at most {MAX_ROWS} rows, got {B}")
    v32 = _host(value).reshape(-1)
    uf, ks = _host(u), _host(mode_index).reshape(-1)
    n_src = uf.shape[0]
    stored = {"old_log_prob": _host(old_log_prob), "advantage": _host(advantage), "returns": _host(returns)}
    if clip_value is not None:
        if old_value is None:
            raise ValueError("ppo loss: clip_value needs old_value")
        stored["old_value"] = _host(old_value)
    if v32.dtype != np.float32 or v32.shape != (B,) or uf.dtype != np.float32 or uf.shape != (n_src, 4) or ks.shape != (n_src,) \
            or any(a.dtype != np.float32 or a.reshape(-1).shape != (n_src,) for a in stored.values()):
        raise ValueError("ppo loss: value must be float32 [B], u float32 [n_src, 4], the other stored blocks float32 [n_src]")
    if index is None:
        if n_src != B:
            raise ValueError(f"ppo loss: without an index the stored blocks hold one entry per row ({B}), got {n_src}")
        src = np.arange(B, dtype=np.int64)
    else:
        src = _host(index).reshape(-1).astype(np.int64)
        if src.shape != (B,):
            raise ValueError(f"ppo loss: index must have {B} entries")
    clip, vf_coef, ent_coef = float(clip), float(vf_coef), float(ent_coef)
    cv = 0.0 if clip_value is None else float(clip_value)
    if not all(math.isfinite(x) for x in (clip, vf_coef, ent_coef, cv)) or clip < 0.0 or cv < 0.0:
        raise ValueError("ppo loss: clip, vf_coef, ent_coef and clip_value must be finite, clip and clip_value not negative")
    bad = (src < 0) | (src >= n_src)
    at = np.where(bad, 0, src)  # (a bad row's terms are computed from entry 0 and thrown away)
    live = ~bad
    if valid is not None:
        live = live & (_host(valid).reshape(-1).view(np.uint8)[at] != 0)
    kw = dict(modes=modes, lo=lo, hi=hi, log_span=log_span, u=np.ascontiguousarray(uf[at]), mode_index=ks[at])
    with np.errstate(all="ignore"):
        ev = policy_head_definition(EVALUATE, p, **kw)
        lp = _f32(ev["log_prob64"]).astype(np.float64)
        ent = ev["entropy64"]
        old, A, R = (stored[k].reshape(-1)[at].astype(np.float64) for k in ("old_log_prob", "advantage", "returns"))
        v = v32.astype(np.float64)
        lr = lp - old
        ratio = portable_exp(lr)
        lo_c, hi_c = 1.0 - clip, 1.0 + clip
        rc = np.where(ratio < lo_c, lo_c, np.where(ratio > hi_c, hi_c, ratio))
        s1, s2 = ratio * A, rc * A
        clipped = s2 < s1
        pol = -np.where(clipped, s2, s1)
        dlp = np.where(clipped, 0.0, -(A * ratio))
        kl = (ratio - 1.0) - lr
        cf = np.where((ratio < lo_c) | (ratio > hi_c), 1.0, 0.0)
        e = v - R
        vl, dv = e * e, e
        if clip_value is not None:
            ov = stored["old_value"].reshape(-1)[at].astype(np.float64)
            d = v - ov
            dc = np.where(d < -cv, -cv, np.where(d > cv, cv, d))
            ec = (ov + dc) - R
            vlc = ec * ec
            worse = vlc > vl
            vl, dv = np.where(worse, vlc, vl), np.where(worse, np.where(dc == d, ec, 0.0), dv)
        vloss = 0.5 * vl
        rows7 = np.stack([np.ones(B), np.zeros(B), pol, vloss, ent, kl, cf], axis=1)
        rows7 = np.where(live[:, None], rows7, 0.0)
        rows7[:, 1] = bad
        partials, S = pairwise_sum(rows7)
        n = S[0]
        s = 1.0 / n if n > 0 else 0.0
        pl, vm, em = S[2] * s, S[3] * s, S[4] * s
        stats = np.array([n, S[1], (pl + vf_coef * vm) - ent_coef * em, pl, vm, em, S[5] * s, S[6] * s])
        bw = policy_head_definition(BACKWARD, p, g_log_prob=dlp * s, g_entropy=np.full(B, -ent_coef * s), **kw)
        gp = np.where(live[:, None], bw["grad_params64"], 0.0)
        gv = np.where(live, (vf_coef * dv) * s, 0.0)
    return {"stats": _f64(stats), "partials": _f64(partials), "count": np.array([int(live.sum()), int(bad.sum())], dtype=np.int32),
            "grad_params": _f32(gp), "grad_value": _f32(gv), "grad_params64": gp, "grad_value64": gv,
            "live": live, "ratio": ratio, "clipped": clipped, "summands": rows7}


def device_ppo_loss(desc: "_abi.PpoDesc", device) -> None:
    """`wedm_ppo_loss` on ``device`` and torch's current stream, for callers that hold no environment."""
    from . import _lib

    _lib.call_stateless(_lib.load().wedm_ppo_loss, torch.device(device), C.byref(desc))


class PPOStats:
    """A view of the call's ``[8]`` float64 device tensor with named fields (``n``, ``n_bad``, ``loss``, ``policy_loss``,
    ``value_loss``, ``entropy``, ``approx_kl``, ``clip_fraction``: 0-dim tensors on the device).  It is the `PPOLoss`'s own
    tensor, rewritten by its next call; reading a field synchronises nothing, `as_dict` copies to the host."""

    __slots__ = ("tensor",)

    def __init__(self, tensor: torch.Tensor):
        self.tensor = tensor

    def __getattr__(self, name: str) -> torch.Tensor:
        if name in STAT_NAMES:
            return self.tensor[STAT_NAMES.index(name)]
        raise AttributeError(name)

    def as_dict(self) -> Dict[str, float]:
        return dict(zip(STAT_NAMES, self.tensor.detach().cpu().tolist()))


class _Loss(torch.autograd.Function):
    """The loss as a float32 scalar; its backward multiplies the gradients the call stored by the upstream scalar."""

    @staticmethod
    def forward(ctx, ppo, params, value, kw):
        grads, stats = ppo._run(params, value, **kw)
        ctx.ppo, ctx.version, ctx.shape = ppo, ppo._version, tuple(grads[0].shape)
        return stats.tensor[2].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        ppo, (B, P) = ctx.ppo, ctx.shape
        if ppo._version != ctx.version:
            raise RuntimeError("PPOLoss.loss: the stored gradients were overwritten by a later call of this PPOLoss; call "
                               "backward() on a loss before the next loss() / backward()")
        scaled = ppo._grad[: B * (P + 1)] * g.to(torch.float32)  # grad_params and grad_value lie back to back: one launch
        return None, scaled[: B * P].view(B, P), scaled[B * P:], None


class PPOLoss:
    """``PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.0, clip_value=None)``: PPO's loss over minibatches of a policy whose
    action head is ``head`` (a `PolicyHead`: modes, bounds and ``log_span`` are taken from it at every call).

    ``loss = mean(policy) + vf_coef * mean(value) - ent_coef * mean(entropy)`` over the live rows: ``policy`` the clipped
    surrogate ``-min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)``, ``value`` ``0.5 * (v - R)^2`` (with ``clip_value``:
    the larger of it and the same at ``old_value + clamp(v - old_value, +-clip_value)``), ``entropy`` the head's.  A row
    with ``valid == 0`` -- the step after a done, which `RolloutBuffer` excludes -- takes no part and gets a zero gradient.
    The workspace is allocated here, the gradient buffers grow to the largest minibatch seen; after that a call allocates
    nothing and never synchronises with the host."""

    def __init__(self, head: PolicyHead, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
                 clip_value: Optional[float] = None):
        self.head, self.device = head, head.device
        self._set(clip, vf_coef, ent_coef, clip_value)
        native = head._native
        self._native = native if hasattr(native, "ppo_loss") else None
        kw = dict(device=self.device)
        self._partials = torch.zeros((_abi.NORM_MAX_TILES, _abi.PPO_SUMS), dtype=torch.float64, **kw)
        self._count = torch.zeros(_abi.PPO_COUNT_WORDS, dtype=torch.int32, **kw)
        self._stats = torch.zeros(_abi.PPO_STATS, dtype=torch.float64, **kw)
        self._grad = torch.zeros(0, dtype=torch.float32, **kw)  # [B * P] grad_params, then [B] grad_value
        self._version = 0
        self._keep = None  # the inputs of the launches in flight

    def _set(self, clip, vf_coef, ent_coef, clip_value) -> None:
        clip, vf_coef, ent_coef = float(clip), float(vf_coef), float(ent_coef)
        clip_value = None if clip_value is None else float(clip_value)
        if not all(math.isfinite(x) for x in (clip, vf_coef, ent_coef, 0.0 if clip_value is None else clip_value)):
            raise ValueError("clip, vf_coef, ent_coef and clip_value must be finite")
        if clip < 0.0 or (clip_value is not None and clip_value < 0.0):
            raise ValueError("clip and clip_value must not be negative")
        self.clip, self.vf_coef, self.ent_coef, self.clip_value = clip, vf_coef, ent_coef, clip_value

    # ------------------------------------------------------------------ arguments
    def _check(self, name: str, t, shape, dtypes) -> torch.Tensor:
        if not torch.is_tensor(t) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a {' / '.join(str(d) for d in dtypes)} tensor {list(shape)}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
        if t.device.type != self.device.type or (self.device.index is not None and t.device.index != self.device.index):
            raise ValueError(f"{name} lies on {t.device}, the loss on {self.device}")
        return t.detach().contiguous()

    def _stored(self, B: int, u, mode_index, old_log_prob, advantage, returns, old_value, valid, rollout, index):
        """The stored blocks as contiguous tensors, ``n_src`` and the index."""
        f32 = (torch.float32,)
        if rollout is not None:
            if any(x is not None for x in (u, mode_index, old_log_prob, advantage, returns, old_value, valid)):
                raise ValueError("rollout= replaces the stored tensors: pass either it (with index=) or them")
            if index is None:
                raise ValueError("rollout= needs index=, the minibatch's slice of a permutation of the rollout's steps")
            flat = rollout.flat()
            missing = [k for k in ("action.u", "action.mode_index", "log_prob") if k not in flat]
            if missing:
                raise ValueError(f"the rollout stores no {missing}: add PolicyHead.stored(out) as the action and "
                                 f"extras={{'log_prob': out.log_prob}} (RolloutBuffer(..., extras={{'log_prob': torch.float32}}))")
            u, mode_index, old_log_prob = flat["action.u"], flat["action.mode_index"], flat["log_prob"]
            advantage = flat["advantage_norm"] if "advantage_norm" in flat else flat["advantage"]
            returns, old_value, valid = flat["returns"], flat["value"], flat["valid"]
            if mode_index.dtype != torch.int32:
                raise ValueError(f"the rollout's action.mode_index must be int32, got {mode_index.dtype}")
            n_src = rollout.num_steps * rollout.num_envs
            index = self._check("index", index, (B,), (torch.int64,))
        else:
            if index is not None:
                raise ValueError("index= goes with rollout=")
            if any(x is None for x in (u, mode_index, old_log_prob, advantage, returns)):
                raise ValueError("u, mode_index, old_log_prob, advantage and returns are needed (or rollout= and index=)")
            n_src = B
            if torch.is_tensor(mode_index) and not mode_index.is_floating_point() and mode_index.dtype != torch.int32:
                mode_index = mode_index.to(torch.int32)
        out = {"u": self._check("u", u, (n_src, 4), f32), "mode_index": self._check("mode_index", mode_index, (n_src,), (torch.int32,)),
               "old_log_prob": self._check("old_log_prob", old_log_prob, (n_src,), f32),
               "advantage": self._check("advantage", advantage, (n_src,), f32), "returns": self._check("returns", returns, (n_src,), f32),
               "old_value": None, "valid": None}
        if self.clip_value is not None:
            if old_value is None:
                raise ValueError("clip_value is set: old_value is needed")
            out["old_value"] = self._check("old_value", old_value, (n_src,), f32)
        if valid is not None:
            out["valid"] = self._check("valid", valid, (n_src,), (torch.bool, torch.uint8))
        return out, n_src, index

    # ------------------------------------------------------------------ the call
    def _run(self, params, value, *, u=None, mode_index=None, old_log_prob=None, advantage=None, returns=None, old_value=None,
             valid=None, rollout=None, index=None):
        """One `wedm_ppo_loss`: ((grad_params ``[B, P]``, grad_value ``[B]``), `PPOStats`), the loss's own buffers."""
        head = self.head
        P = head.param_dim
        if torch.is_tensor(params) and params.ndim == 2 and params.shape[0] > MAX_ROWS:
            raise ValueError(f"a minibatch holds at most {MAX_ROWS} rows ({_abi.NORM_MAX_TILES} tiles of {TILE}), got {params.shape[0]}")
        if not torch.is_tensor(params) or params.ndim != 2 or params.shape[0] < 1:
            raise ValueError(f"params must be a float32 tensor [B, {P}]")
        B = params.shape[0]
        p = self._check("params", params, (B, P), (torch.float32,))
        v = self._check("value", value, (B,), (torch.float32,))
        s, n_src, index = self._stored(B, u, mode_index, old_log_prob, advantage, returns, old_value, valid, rollout, index)
        if self._grad.numel() < B * (P + 1):
            self._grad = torch.zeros(B * (P + 1), dtype=torch.float32, device=self.device)
        gp, gv = self._grad[: B * P].view(B, P), self._grad[B * P: B * (P + 1)]
        if self._native is not None:
            ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
            d = _abi.PpoDesc(params=p.data_ptr(), value=v.data_ptr(), index=ptr(index), u=ptr(s["u"]), mode_index=ptr(s["mode_index"]),
                             old_log_prob=ptr(s["old_log_prob"]), advantage=ptr(s["advantage"]), returns=ptr(s["returns"]),
                             old_value=ptr(s["old_value"]), valid=ptr(s["valid"]), grad_params=gp.data_ptr(), grad_value=gv.data_ptr(),
                             partials=self._partials.data_ptr(), stats=self._stats.data_ptr(), count=self._count.data_ptr(),
                             param_stride=P, grad_stride=P, n_src=n_src, clip=self.clip, vf_coef=self.vf_coef, ent_coef=self.ent_coef,
                             clip_value=0.0 if self.clip_value is None else self.clip_value, n_modes=len(head.modes), rows=B,
                             flags=0 if self.clip_value is None else _abi.PPO_CLIP_VALUE)
            d.lo[:], d.hi[:], d.log_span[:] = head._lo, head._hi, head._log_span
            with torch.cuda.device(p.device):
                self._native.ppo_loss(d)
            self._keep = (p, v, index, s)  # the launches are asynchronous: their inputs live until the next call
        else:
            res = ppo_loss_definition(p, v, modes=head.modes, lo=head._lo, hi=head._hi, log_span=head._log_span, index=index,
                                      clip=self.clip, vf_coef=self.vf_coef, ent_coef=self.ent_coef, clip_value=self.clip_value,
                                      **{k: t for k, t in s.items() if t is not None})
            gp.copy_(torch.from_numpy(res["grad_params"]))
            gv.copy_(torch.from_numpy(res["grad_value"]))
            self._stats.copy_(torch.from_numpy(res["stats"]))
            self._partials[: res["partials"].shape[0]].copy_(torch.from_numpy(res["partials"]))
            self._count.copy_(torch.from_numpy(res["count"]))
        self._version += 1
        return (gp, gv), PPOStats(self._stats)

    def backward(self, params: torch.Tensor, value: torch.Tensor, **kw) -> PPOStats:
        """The loss's gradient into whatever ``params`` (float32 ``[B, param_dim]``) and ``value`` (float32 ``[B]``) were
        computed from: one `wedm_ppo_loss`, then ``torch.autograd.backward((params, value), (grad_params, grad_value))`` --
        no pass over ``[B, P]`` scales by an upstream gradient.  Either the stored tensors of the minibatch, gathered:
        ``u=, mode_index=, old_log_prob=, advantage=, returns=`` (and ``old_value=`` with ``clip_value``, ``valid=`` or
        None: every row counts); or ``rollout=buf, index=idx``: the buffer's blocks (``action.u``, ``action.mode_index``, the
        ``log_prob`` extra, ``advantage_norm`` -- ``advantage`` where the buffer does not normalise --, ``returns``, ``value``
        as ``old_value``, ``valid``) are read in place at ``idx`` (int64 ``[B]``, a slice of a permutation of the ``T * N``
        steps), and only ``obs[idx]`` is gathered by the caller, for the network.  Returns the `PPOStats` of the minibatch:
        a view of a device tensor, no host synchronisation.  The float32 rounding of the log-probability is treated as the
        identity in the gradient, as is usual."""
        (gp, gv), stats = self._run(params, value, **kw)
        pairs = [(t, g) for t, g in ((params, gp), (value, gv)) if t.requires_grad]  # (neither: the statistics alone)
        if pairs:
            torch.autograd.backward(*zip(*pairs))
        return stats

    def loss(self, params: torch.Tensor, value: torch.Tensor, **kw) -> torch.Tensor:
        """The loss as a float32 scalar tensor, for users who add terms of their own: the same arguments and the same one
        call as `backward`; differentiable through a ``torch.autograd.Function`` whose backward multiplies the stored
        gradients by the upstream scalar -- one torch launch over ``[B, param_dim + 1]`` that `backward` does not spend.
        The stored gradients are this `PPOLoss`'s own buffers: run the scalar's ``backward()`` before the next call.
        `stats` holds the statistics of the last call."""
        return _Loss.apply(self, params, value, kw)

    @property
    def stats(self) -> PPOStats:
        """The statistics of the last call."""
        return PPOStats(self._stats)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        return {"clip": self.clip, "vf_coef": self.vf_coef, "ent_coef": self.ent_coef, "clip_value": self.clip_value}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        self._set(sd["clip"], sd["vf_coef"], sd["ent_coef"], sd["clip_value"])
