"""Policy action head on the device: sample, log-probability, gradient.

What stands between a policy network's output row and `WireEDMVectorEnv.step`, and what an on-policy update (PPO, A2C)
evaluates again at the stored actions.  A row of ``8 + M`` float32 parameters -- four means, four log standard deviations,
``M`` logits -- describes four tanh-squashed Gaussians mapped affinely to the bounds of ``servo``, ``target_voltage``,
``ON_time`` and ``OFF_time``, and a categorical over ``M`` of the current modes that have crater data.  `wedm_policy_head`
(include/wedm_hip.h, which holds the definition with every rounding) draws the action, or evaluates its log-probability and
entropy, or their gradient, in one launch each.  A draw is a pure function of ``(seed, global environment id, step number,
row)``: Philox4x32-10 of the step kernels on streams of its own, the kernels' portable exp and log, float64 with nothing
fused -- so the actions of a rollout carry the same bits over 1 or 8 devices, batch splits and checkpoints, as its
trajectories already do.

`policy_head_definition` is that definition on host data in NumPy float64: the path of backends without the call (the CPU
oracle backends of the tests) and what the kernels are checked against, bit for bit.  `PolicyHead` owns the tensors.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .core.tables import VALID_CRATER_MODES
from .envs.wire_edm import DeviceAction
from .normalize import _host
from .randomize import philox4x32_10

SAMPLE, EVALUATE, BACKWARD = _abi.HEAD_SAMPLE, _abi.HEAD_EVALUATE, _abi.HEAD_BACKWARD
LEAVES = ("servo", "target_voltage", "ON_time", "OFF_time")  # the continuous components, in the descriptor's order
LN2, HALF_LOG_2PI, HALF_LOG_2PIE = 0.6931471805599453, 0.9189385332046727, 1.4189385332046727
_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ portable math, normals
def portable_exp(x) -> np.ndarray:
    """`portable_exp` of the kernels (csrc/wedm_portable.h) and the CPU oracle, element-wise on float64, bit for bit."""
    x = np.asarray(x, dtype=np.float64)
    ln2hi, ln2lo, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    with np.errstate(all="ignore"):
        nan, over, under = x != x, x > 709.0, x < -708.0
        inside = ~(nan | over | under)
        xs = np.where(inside, x, 0.0)  # (the other lanes take the early returns below)
        ax = np.abs(xs)
        big = ax > 0.34657359027997264
        k = np.where(big, np.trunc(invln2 * xs + np.where(xs < 0, -0.5, 0.5)), 0.0)
        hi = np.where(big, xs - k * ln2hi, xs)
        lo = np.where(big, k * ln2lo, 0.0)
        r = np.where(big, hi - lo, xs)
        t = r * r
        c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
        near = 1.0 - ((r * c) / (c - 2.0) - r)
        y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
        scale = ((k.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
        out = np.where(k == 0.0, near, y * scale)
        out = np.where(~big & (ax < 3.725290298461914e-09), 1.0 + xs, out)
        out = np.where(under, 0.0, np.where(over, np.inf, out))
        return np.where(nan, x, out)


def portable_log(x) -> np.ndarray:
    """`portable_log` of the kernels and the CPU oracle (positive normal arguments), element-wise on float64, bit for bit."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    ln2hi, ln2lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    ux = x.view(np.uint64)
    hx = ux >> np.uint64(32)
    k = (hx >> np.uint64(20)).astype(np.int64) - 1023
    hx = hx & np.uint64(0x000FFFFF)
    i = (hx + np.uint64(0x95F64)) & np.uint64(0x100000)
    ux = ((hx | (i ^ np.uint64(0x3FF00000))) << np.uint64(32)) | (ux & _M32)
    k = k + (i >> np.uint64(20)).astype(np.int64)
    with np.errstate(all="ignore"):
        f = ux.view(np.float64) - 1.0
        dk = k.astype(np.float64)
        hfsq = 0.5 * f * f
        s = f / (2.0 + f)
        z = s * s
        w = z * z
        t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
        t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
        R = t2 + t1
        return dk * ln2hi - ((hfsq - (s * (hfsq + R) + dk * ln2lo)) - f)


def _head_log(x: np.ndarray) -> np.ndarray:
    """``plog`` of the definition: `portable_log` reads its argument's bits, so a NaN stays the NaN it is."""
    return np.where(x != x, x, portable_log(np.where(x != x, 1.0, x)))


def _f32(x: np.ndarray) -> np.ndarray:
    """``f32`` of the definition: the rounding of every float32 the call stores; a NaN becomes 0x7FC00000."""
    with np.errstate(all="ignore"):
        return np.where(x != x, _NAN32, x.astype(np.float32))


def polar_normal(key: Tuple[int, int], time, episode, gid, stream_base: int = 1) -> np.ndarray:
    """`philox_std_normal` of the kernels: Marsaglia's polar method on the 53-bit pairs of Philox streams ``stream_base +
    j``, the first attempt ``j < 64`` whose point lies inside the unit circle (none: 0.0).  ``time``, ``episode`` and
    ``gid`` broadcast against each other."""
    time, episode, gid = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) & _M32 for a in (time, episode, gid)))
    out, pending = np.zeros(time.shape, dtype=np.float64), np.ones(time.shape, dtype=bool)
    for j in range(64):
        if not pending.any():
            break
        w = philox4x32_10((time[pending], episode[pending], gid[pending], (stream_base + j) & 0xFFFFFFFF), key)
        x, y, z, ww = (a.astype(np.uint64) for a in w)
        a = ((x >> np.uint64(5)).astype(np.float64) * 67108864.0 + (y >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
        b = ((z >> np.uint64(5)).astype(np.float64) * 67108864.0 + (ww >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
        v1, v2 = 2.0 * a - 1.0, 2.0 * b - 1.0
        q = v1 * v1 + v2 * v2
        ok = (q < 1.0) & (q != 0.0)
        qs = np.where(ok, q, 0.5)
        val = v1 * np.sqrt(-2.0 * portable_log(qs) / qs)
        at = np.flatnonzero(pending.reshape(-1))
        out.reshape(-1)[at[ok]] = val[ok]
        pending.reshape(-1)[at[ok]] = False
    return out


# ------------------------------------------------------------------------------------------------ the definition
def policy_head_definition(op: int, params, *, modes: Sequence[int], lo, hi, log_span=None, u=None, mode_index=None,
                           g_log_prob=None, g_entropy=None, seed: int = 0, t: int = 0, env_id_offset: int = 0,
                           deterministic: bool = False) -> Dict[str, np.ndarray]:
    """The definition of `wedm_policy_head` (include/wedm_hip.h) on host data, NumPy float64 with the header's roundings.

    ``params``: float32 ``[rows, >= 8 + M]`` (tensor on any device, or array; columns ``[0, 8 + M)`` are read); ``modes``:
    the ``M`` mode numbers; ``lo`` / ``hi`` / ``log_span``: four values each (``log_span`` defaults to ``log(hi - lo)``).
    ``SAMPLE`` draws with ``seed``, step number ``t`` and global ids ``env_id_offset + row`` (``deterministic``: the means
    and the first largest logit) and returns ``action`` (float64 ``[rows, 4]``), ``current_mode``, ``u`` (float32 ``[rows,
    4]``), ``mode_index`` (int32), ``log_prob`` and ``entropy``; ``EVALUATE`` takes ``u`` and ``mode_index`` and returns the
    last two; ``BACKWARD`` also takes ``g_log_prob`` and ``g_entropy`` (None: zeros) and returns ``grad_params`` (float32
    ``[rows, 8 + M]``).  Beside the float32 outputs the unrounded float64 values are returned as ``log_prob64``,
    ``entropy64`` and ``grad_params64``.  The entropy is that of the base Gaussians plus the categorical's, not of the
    squashed variables.  Nothing that is passed in is modified."""
    modes = np.asarray(list(modes), dtype=np.int32)
    M = int(modes.shape[0])
    if not 1 <= M <= _abi.HEAD_MAX_MODES:
        raise ValueError(f"policy head: {M} modes, outside [1, {_abi.HEAD_MAX_MODES}]")
    P = 8 + M
    p = _host(params)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < P or p.shape[0] < 1:
        raise ValueError(f"policy head: params must be float32 [rows >= 1, >= {P}], got {p.dtype} {list(p.shape)}")
    rows = p.shape[0]
    lo, hi = (np.asarray(a, dtype=np.float64).reshape(4) for a in (lo, hi))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError("policy head: bounds must be finite with lo < hi")
    with np.errstate(all="ignore"):
        log_span = np.log(hi - lo) if log_span is None else np.asarray(log_span, dtype=np.float64).reshape(4)
        mu, ls, l = (p[:, a:b].astype(np.float64) for a, b in ((0, 4), (4, 8), (8, P)))
        sigma = portable_exp(ls)
        out: Dict[str, np.ndarray] = {}
        key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        t0, t1 = int(t) & 0xFFFFFFFF, (int(t) >> 32) & 0xFFFFFFFF
        gid = (np.uint64(int(env_id_offset) & 0xFFFFFFFF) + np.arange(rows, dtype=np.uint64)) & _M32
        if op == SAMPLE:
            if deterministic:
                uf = p[:, 0:4].copy()
            else:
                n = np.stack([polar_normal(key, t0, t1, gid, _abi.HEAD_STREAM0 + 64 * i) for i in range(4)], axis=1)
                uf = _f32(mu + sigma * n)
        else:
            uf = _host(u)
            if uf.dtype != np.float32 or uf.shape != (rows, 4):
                raise ValueError(f"policy head: u must be float32 [{rows}, 4], got {uf.dtype} {list(uf.shape)}")
            k = np.clip(_host(mode_index).reshape(-1).astype(np.int64), 0, M - 1)
            if k.shape != (rows,):
                raise ValueError(f"policy head: mode_index must have {rows} entries")
        ud = uf.astype(np.float64)

        # the continuous components
        z = (ud - mu) / sigma
        a = np.abs(ud)
        e = portable_exp(-2.0 * a)
        s = np.where(ud >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
        x = lo + (hi - lo) * s
        x = np.where(x > lo, x, lo)
        action = np.where(x < hi, x, hi)
        logjac = ((log_span + LN2) - 2.0 * a) - 2.0 * _head_log(1.0 + e)
        c = (((-0.5 * z) * z - ls) - HALF_LOG_2PI) - logjac

        # the categorical
        m = l[:, 0].copy()
        for j in range(1, M):
            m = np.where(l[:, j] > m, l[:, j], m)
        d = l - m[:, None]
        w = portable_exp(d)
        W, S = np.zeros(rows), np.zeros(rows)
        for j in range(M):
            W = W + w[:, j]
            S = S + w[:, j] * d[:, j]
        logW = _head_log(W)
        H = logW - S / W

        if op == SAMPLE:
            if deterministic:
                k, best = np.zeros(rows, dtype=np.int64), l[:, 0].copy()
                for j in range(1, M):
                    better = l[:, j] > best
                    best, k = np.where(better, l[:, j], best), np.where(better, j, k)
            else:
                word = philox4x32_10((t0, t1, gid, (_abi.HEAD_STREAM0 + 256) & 0xFFFFFFFF), key)[0]
                tau = ((word.astype(np.float64) + 0.5) * 2.3283064365386963e-10) * W
                k, run, found = np.full(rows, M - 1, dtype=np.int64), np.zeros(rows), np.zeros(rows, dtype=bool)
                for j in range(M):
                    run = run + w[:, j]
                    hit = ~found & (run > tau)
                    k, found = np.where(hit, j, k), found | hit
            out.update(action=action, current_mode=modes[k], u=uf, mode_index=k.astype(np.int32))
        at = np.arange(rows)
        if op != BACKWARD:
            lp = (((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]) + (d[at, k] - logW)
            t4 = ls + HALF_LOG_2PIE
            ent = (((t4[:, 0] + t4[:, 1]) + t4[:, 2]) + t4[:, 3]) + H
            out.update(log_prob=_f32(lp), entropy=_f32(ent), log_prob64=lp, entropy64=ent)
        else:
            glp = _host(g_log_prob).reshape(-1).astype(np.float64)[:, None]
            gen = np.zeros((rows, 1)) if g_entropy is None else _host(g_entropy).reshape(-1).astype(np.float64)[:, None]
            pj, logp = w / W[:, None], d - logW[:, None]
            ind = (np.arange(M)[None, :] == k[:, None]).astype(np.float64)
            grad = np.concatenate([glp * (z / sigma), glp * (z * z - 1.0) + gen,
                                   glp * (ind - pj) - gen * (pj * (logp + H[:, None]))], axis=1)
            out.update(grad_params=_f32(grad), grad_params64=grad)
    return out


def device_policy_head(desc: "_abi.HeadDesc", device) -> None:
    """`wedm_policy_head` on ``device`` and torch's current stream, for callers that hold no environment."""
    from . import _lib

    _lib.call_stateless(_lib.load().wedm_policy_head, torch.device(device), C.byref(desc))


# ------------------------------------------------------------------------------------------------ the head
class HeadSample:
    """What `PolicyHead.sample` returns: ``action`` (a `DeviceAction`), ``u`` (float32 ``[N, 4]``, the pre-squash values),
    ``mode_index`` (int32 ``[N]``), ``log_prob`` and ``entropy`` (float32 ``[N]``) -- the head's own tensors."""

    __slots__ = ("action", "u", "mode_index", "log_prob", "entropy")

    def __init__(self, action, u, mode_index, log_prob, entropy):
        self.action, self.u, self.mode_index, self.log_prob, self.entropy = action, u, mode_index, log_prob, entropy


class _Evaluate(torch.autograd.Function):
    """``(log_prob, entropy)`` at stored actions; the gradient with respect to ``params`` is one ``BACKWARD`` call."""

    @staticmethod
    def forward(ctx, head, params, u, mode_index):
        ctx.set_materialize_grads(False)
        ctx.head = head
        ctx.save_for_backward(params, u, mode_index)
        return head._call(EVALUATE, params, u, mode_index)

    @staticmethod
    def backward(ctx, g_log_prob, g_entropy):
        params, u, mode_index = ctx.saved_tensors
        if g_log_prob is None:
            g_log_prob = torch.zeros(params.shape[0], dtype=torch.float32, device=params.device)
        grad = ctx.head._call(BACKWARD, params, u, mode_index, g_log_prob.to(torch.float32).contiguous(),
                              None if g_entropy is None else g_entropy.to(torch.float32).contiguous())
        return None, grad, None, None


class PolicyHead:
    """``PolicyHead(env_or_vec, modes=VALID_CRATER_MODES, bounds=None, seed=0)``: the action head of a policy over a
    `WireEDMEnv` or `WireEDMVectorEnv`.

    ``modes``: the current modes the categorical chooses among, a non-empty subset of `VALID_CRATER_MODES` without
    repeats; logit ``j`` belongs to ``modes[j]``.  ``bounds``: ``{leaf: (lo, hi)}`` for any of ``servo``,
    ``target_voltage``, ``ON_time``, ``OFF_time``, inside the action space's, which are the default.  ``param_dim`` is
    ``8 + len(modes)``: a row is ``[mean x 4, log_std x 4, logit x M]``.  ``log_std`` is used as given: a trainer clamps it
    in its own module, where the clamp's gradient belongs.

    The entropy returned by `sample` and `evaluate` is that of the base Gaussians plus the categorical's, not of the
    squashed variables (which has no closed form): the usual entropy-bonus surrogate."""

    def __init__(self, env_or_vec, modes: Sequence[int] = VALID_CRATER_MODES, bounds: Optional[Dict[str, Tuple[float, float]]] = None,
                 seed: int = 0):
        env = getattr(env_or_vec, "env", env_or_vec)
        self.num_envs, self.device = int(env.num_envs), torch.device(env.device)
        self.env_id_offset = int(env.env_id_offset) & 0xFFFFFFFF
        backend = getattr(env, "_backend", None)
        self._native = backend if hasattr(backend, "policy_head") else None
        gc = env.action_space["generator_control"]
        self._space = {"servo": env.action_space["servo"], **{k: gc[k] for k in LEAVES[1:]}}
        self.seed, self.t = int(seed) & (2 ** 64 - 1), 0
        self._set(modes, bounds)
        N, kw = self.num_envs, dict(device=self.device)
        leaves = [torch.zeros(N, dtype=torch.float64, **kw) for _ in LEAVES]
        self._out = HeadSample(DeviceAction(*leaves, torch.full((N,), self.modes[0], dtype=torch.int32, **kw)),
                               torch.zeros((N, 4), dtype=torch.float32, **kw), torch.zeros(N, dtype=torch.int32, **kw),
                               torch.zeros(N, dtype=torch.float32, **kw), torch.zeros(N, dtype=torch.float32, **kw))
        self._keep = None  # the input of the launch in flight

    def _set(self, modes, bounds) -> None:
        modes = [int(m) for m in modes]
        if not modes or len(set(modes)) != len(modes) or any(m not in VALID_CRATER_MODES for m in modes):
            raise ValueError(f"modes must be a non-empty subset of {list(VALID_CRATER_MODES)} without repeats, got {modes}")
        given = dict(bounds or {})
        unknown = sorted(set(given) - set(LEAVES))
        if unknown:
            raise ValueError(f"bounds: unknown leaves {unknown}; the continuous leaves are {list(LEAVES)}")
        self.bounds: Dict[str, Tuple[float, float]] = {}
        for name in LEAVES:
            low, high = float(np.min(self._space[name].low)), float(np.max(self._space[name].high))
            lo, hi = (float(v) for v in given.get(name, (low, high)))
            if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
                raise ValueError(f"bounds of {name!r} must be finite with lo < hi, got ({lo}, {hi})")
            if lo < low or hi > high:
                raise ValueError(f"bounds of {name!r} ({lo}, {hi}) reach outside the action space's ({low}, {high})")
            self.bounds[name] = (lo, hi)
        self.modes = tuple(modes)
        self.param_dim = 8 + len(modes)
        self._lo = [self.bounds[k][0] for k in LEAVES]
        self._hi = [self.bounds[k][1] for k in LEAVES]
        self._log_span = [math.log(h - l) for l, h in zip(self._lo, self._hi)]  # computed once; device and definition use it

    # ------------------------------------------------------------------ the call
    def _desc(self, op: int, rows: int) -> "_abi.HeadDesc":
        d = _abi.HeadDesc(op=op, rows=rows, n_modes=len(self.modes), param_stride=self.param_dim, grad_stride=self.param_dim,
                          seed=self.seed, t=self.t, env_id_offset=self.env_id_offset)
        d.lo[:], d.hi[:], d.log_span[:] = self._lo, self._hi, self._log_span
        d.modes[: len(self.modes)] = self.modes
        return d

    def _definition(self, op: int, params, **kw) -> Dict[str, np.ndarray]:
        return policy_head_definition(op, params, modes=self.modes, lo=self._lo, hi=self._hi, log_span=self._log_span,
                                      seed=self.seed, t=self.t, env_id_offset=self.env_id_offset, **kw)

    def _check_params(self, params, rows: Optional[int]) -> torch.Tensor:
        if not torch.is_tensor(params) or params.dtype != torch.float32 or params.ndim != 2 or params.shape[1] != self.param_dim \
                or params.shape[0] < 1 or (rows is not None and params.shape[0] != rows):
            raise ValueError(f"params must be a float32 tensor [{'B' if rows is None else rows}, {self.param_dim}], got "
                             f"{getattr(params, 'dtype', type(params).__name__)} {list(getattr(params, 'shape', []))}")
        return params.detach().contiguous()

    def _call(self, op: int, params, u, mode_index, g_log_prob=None, g_entropy=None):
        """EVALUATE -> (log_prob, entropy), BACKWARD -> grad_params, on the device of ``params``."""
        rows, dev = params.shape[0], params.device
        if self._native is not None:
            d = self._desc(op, rows)
            d.params, d.u, d.mode_index = params.data_ptr(), u.data_ptr(), mode_index.data_ptr()
            if op == EVALUATE:
                out = (torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev))
                d.log_prob, d.entropy = out[0].data_ptr(), out[1].data_ptr()
            else:
                out = torch.empty((rows, self.param_dim), dtype=torch.float32, device=dev)
                d.g_log_prob, d.grad_params = g_log_prob.data_ptr(), out.data_ptr()
                d.g_entropy = None if g_entropy is None else g_entropy.data_ptr()
            with torch.cuda.device(dev):
                self._native.policy_head(d)
            return out
        res = self._definition(op, params, u=u, mode_index=mode_index, g_log_prob=g_log_prob, g_entropy=g_entropy)
        if op == EVALUATE:
            return torch.from_numpy(res["log_prob"]).to(dev), torch.from_numpy(res["entropy"]).to(dev)
        return torch.from_numpy(res["grad_params"]).to(dev)

    def sample(self, params: torch.Tensor, deterministic: bool = False) -> HeadSample:
        """The action of every environment from its row of ``params`` (float32 ``[num_envs, param_dim]`` on the head's
        device): one launch, no allocation after the first call and no host synchronisation.  Returns the head's own
        `HeadSample`, the same object at every call, rewritten in place: ``action`` goes to ``vec.step``, `stored` into the
        rollout.  A non-deterministic call draws with the step number `t` and advances it; ``deterministic=True`` takes the
        means and the first largest logit and draws nothing."""
        params = self._check_params(params, self.num_envs)
        if params.device.type != self.device.type:
            raise ValueError(f"params lie on {params.device}, the head on {self.device}")
        o = self._out
        if self._native is not None:
            d = self._desc(SAMPLE, self.num_envs)
            d.flags = _abi.HEAD_DETERMINISTIC if deterministic else 0
            d.params, d.u, d.mode_index = params.data_ptr(), o.u.data_ptr(), o.mode_index.data_ptr()
            a = o.action
            d.action[:] = [a.servo.data_ptr(), a.target_voltage.data_ptr(), a.on_time.data_ptr(), a.off_time.data_ptr()]
            d.current_mode, d.log_prob, d.entropy = a.current_mode.data_ptr(), o.log_prob.data_ptr(), o.entropy.data_ptr()
            self._native.policy_head(d)
            self._keep = params  # the launch is asynchronous: its input lives until the next call
        else:
            res = self._definition(SAMPLE, params, deterministic=deterministic)
            a = o.action
            for i, leaf in enumerate((a.servo, a.target_voltage, a.on_time, a.off_time)):
                leaf.copy_(torch.from_numpy(np.ascontiguousarray(res["action"][:, i])))
            a.current_mode.copy_(torch.from_numpy(res["current_mode"]))
            for name in ("u", "mode_index", "log_prob", "entropy"):
                getattr(o, name).copy_(torch.from_numpy(res[name]))
        if not deterministic:
            self.t = (self.t + 1) & (2 ** 64 - 1)
        return o

    @staticmethod
    def stored(out: HeadSample) -> Dict[str, torch.Tensor]:
        """``{"u": ..., "mode_index": ...}``: what goes into `RolloutBuffer.add` as the action (with
        ``extras={"log_prob": out.log_prob}``), and later into `evaluate`."""
        return {"u": out.u, "mode_index": out.mode_index}

    def evaluate(self, params: torch.Tensor, u: torch.Tensor, mode_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(log_prob, entropy)`` (float32 ``[B]``) of the stored actions ``u`` (float32 ``[B, 4]``) and ``mode_index``
        (integer ``[B]``) under ``params`` (float32 ``[B, param_dim]``, made contiguous if it is not), differentiable with
        respect to ``params`` through one ``BACKWARD`` launch.  At the sampling parameters ``log_prob`` has the bits that
        `sample` returned."""
        checked = self._check_params(params, None)
        rows = checked.shape[0]
        if not torch.is_tensor(u) or u.dtype != torch.float32 or tuple(u.shape) != (rows, 4):
            raise ValueError(f"u must be a float32 tensor [{rows}, 4]")
        if not torch.is_tensor(mode_index) or mode_index.is_floating_point() or tuple(mode_index.shape) != (rows,):
            raise ValueError(f"mode_index must be an integer tensor [{rows}]")
        if u.device != checked.device or mode_index.device != checked.device or checked.device.type != self.device.type:
            raise ValueError(f"params, u and mode_index must lie on one device of the head's kind ({self.device.type})")
        return _Evaluate.apply(self, params if params.is_contiguous() else params.contiguous(), u.detach().contiguous(),
                               mode_index.detach().to(torch.int32).contiguous())

    # ------------------------------------------------------------------ seed, checkpoints
    def reseed(self, seed: int) -> None:
        """A new seed, and the step number back at 0."""
        self.seed, self.t = int(seed) & (2 ** 64 - 1), 0

    def state_dict(self) -> Dict[str, Any]:
        return {"seed": self.seed, "t": self.t, "modes": list(self.modes), "bounds": {k: tuple(v) for k, v in self.bounds.items()}}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Seed, step number, modes and bounds of `state_dict`: the next `sample` draws what the saved head's would have."""
        self._set(sd["modes"], sd["bounds"])
        self.seed, self.t = int(sd["seed"]) & (2 ** 64 - 1), int(sd["t"])
