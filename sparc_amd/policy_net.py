"""The actor-critic network on the device, forward and backward defined to the bit.

The link between an observation and the head's parameter row: a two-hidden-layer MLP whose every product is a k-ordered
chain of float32 fused multiply-adds and whose gradient is summed over the rows by a fixed tree (include/wedm_hip.h,
`wedm_policy_net`, holds the definition with every rounding).  gfx950's float32 matrix instructions compute exactly such
chains, so the kernels of csrc/wedm_policy_net.h and the NumPy definition below agree on every bit, at every batch size,
batch split and launch shape -- which a chain of library GEMMs does not promise.  A rollout's observations are read in place
through an index, so an update gathers nothing.

`policy_net_reference` is the definition on host data (its float32 fma is built from float64 with a rounding to odd): the
path of backends without the call (the CPU oracle backends of the tests) and what the kernels are checked against.
`PolicyNet` owns ``theta``, the outputs and the workspace.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .normalize import _host

TILE, CHUNK = _abi.NORM_TILE, 64
MAX_ROWS = _abi.NORM_MAX_TILES * TILE
ACTIVATIONS = _abi.NET_ACTIVATIONS
_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
_FMAX = np.float32(np.finfo(np.float32).max)
_h = lambda s: np.float32(float.fromhex(s))   # noqa: E731
# the constants of WEDM_NET_TANH, as the header writes them
_LOG2E, _MAGIC, _LN2_HI, _LN2_LO = _h("0x1.715476p+0"), np.float32(12582912.0), _h("-0x1.62e400p-1"), _h("-0x1.7f7d1cp-20")
_POLY = tuple(_h(s) for s in ("0x1.a01a02p-16", "0x1.a01a02p-13", "0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5",
                              "0x1.555556p-3", "0x1p-1"))


def _canon(x: np.ndarray) -> np.ndarray:
    """Every float32 the call stores: a NaN becomes 0x7FC00000."""
    return np.where(x != x, _NAN32, x).astype(np.float32)


def fma32(a, b, c) -> np.ndarray:
    """``fmaf(a, b, c)`` on float32 arrays (broadcast), one rounding: the product is exact in float64, TwoSum gives the
    residual of its float64 sum with ``c``, an inexact sum is rounded to odd in its 53 bits, one cast to float32 follows."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0.0) & ((np.asarray(s).view(np.int64) & 1) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return np.asarray(s).astype(np.float32)


def clean32(o: np.ndarray) -> np.ndarray:
    """The definition's input cleaning: ``torch.nan_to_num`` with its defaults."""
    o = np.asarray(o, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where(o != o, np.float32(0.0), np.where(o < -_FMAX, -_FMAX, np.where(o > _FMAX, _FMAX, o))).astype(np.float32)


def tanh32(a: np.ndarray) -> np.ndarray:
    """WEDM_NET_TANH of include/wedm_hip.h, step for step, on a float32 array."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(all="ignore"):
        ua = a.view(np.uint32)
        m = (ua & np.uint32(0x7FFFFFFF)).view(np.float32)
        z = m + m
        t = fma32(z, _LOG2E, _MAGIC)
        n = t - _MAGIC
        r = fma32(n, _LN2_HI, z)
        r = fma32(n, _LN2_LO, r)
        p = fma32(r, _POLY[0], _POLY[1])
        for c in _POLY[2:]:
            p = fma32(r, p, c)
        q = fma32(r * r, p, r)
        s = ((np.ascontiguousarray(t).view(np.uint32) << np.uint32(23)) + np.uint32(0x3F800000)).view(np.float32)
        e = fma32(s, q, s - one)
        d = e + two
        g = np.where(m < np.float32(0.5), e / d, one - two / d)
        g = np.where(m > np.float32(10.0), one, g).astype(np.float32)
        return (np.ascontiguousarray(g).view(np.uint32) | (ua & np.uint32(0x80000000))).view(np.float32)


def _act(a: np.ndarray, activation: str) -> np.ndarray:
    return tanh32(a) if activation == "tanh" else np.where(a > 0, a, np.float32(0.0)).astype(np.float32)


def _dact(h: np.ndarray, activation: str) -> np.ndarray:
    if activation == "tanh":
        return fma32(-h, h, np.float32(1.0))
    return np.where(h > 0, np.float32(1.0), np.float32(0.0)).astype(np.float32)


def layout(D: int, hidden: Sequence[int], n_modes: int) -> Dict[str, Tuple[int, Tuple[int, ...]]]:
    """name -> (offset, shape) of ``W1, b1, W2, b2, W3, b3`` in ``theta``, and ``"n_theta"`` -> (size, ())."""
    H1, H2 = (int(h) for h in hidden)
    O = 8 + int(n_modes) + 1
    out, at = {}, 0
    for name, shape in (("W1", (D, H1)), ("b1", (H1,)), ("W2", (H1, H2)), ("b2", (H2,)), ("W3", (H2, O)), ("b3", (O,))):
        out[name] = (at, shape)
        at += int(np.prod(shape))
    out["n_theta"] = (at, ())
    return out


def check_dims(D: int, hidden: Sequence[int], n_modes: int, activation: str) -> None:
    hidden = tuple(int(h) for h in hidden)
    if not 1 <= int(D) <= _abi.NORM_MAX_COLUMNS:
        raise ValueError(f"policy net: obs_dim must lie in [1, {_abi.NORM_MAX_COLUMNS}], got {D}")
    if len(hidden) != 2 or any(h < 16 or h > _abi.NET_MAX_HIDDEN or h % 16 for h in hidden):
        raise ValueError(f"policy net: hidden must be two multiples of 16 in [16, {_abi.NET_MAX_HIDDEN}], got {hidden}")
    if not 1 <= int(n_modes) <= _abi.HEAD_MAX_MODES:
        raise ValueError(f"policy net: n_modes must lie in [1, {_abi.HEAD_MAX_MODES}], got {n_modes}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"policy net: activation must be one of {ACTIVATIONS}, got {activation!r}")


def layer32(x: np.ndarray, W: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The definition's layer on ``[rows, K]``: ``a_j = b_j``, then ``a_j = fma(x_k, W[k][j], a_j)`` for k ascending."""
    a = np.broadcast_to(b.astype(np.float32), (x.shape[0], W.shape[1])).copy()
    for k in range(W.shape[0]):
        a = fma32(x[:, k, None], W[None, k, :], a)
    return a


def back32(g: np.ndarray, W: np.ndarray) -> np.ndarray:
    """``dh_k``: the chain from +0.0 over j ascending of ``fma(g_j, W[k][j], .)``, on ``[rows, N]``."""
    dh = np.zeros((g.shape[0], W.shape[0]), dtype=np.float32)
    for j in range(W.shape[1]):
        dh = fma32(g[:, j, None], W[None, :, j], dh)
    return dh


def tree32(nodes: np.ndarray, levels: Optional[int] = None) -> np.ndarray:
    """The definition's tree over axis 0 with plain float32 additions, the lower index on the left; a node without a
    right child is its left child unchanged.  ``levels``: stop after that many levels (None: down to one node)."""
    nodes = np.asarray(nodes, dtype=np.float32)
    with np.errstate(all="ignore"):
        while nodes.shape[0] > 1 and (levels is None or levels > 0):
            n = nodes.shape[0]
            pairs = nodes[0:n - (n & 1):2] + nodes[1::2]
            nodes = np.concatenate([pairs, nodes[n - 1:]], axis=0) if n & 1 else pairs
            levels = None if levels is None else levels - 1
    return nodes


def rowsum32(u: np.ndarray, v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The definition's SUM_r (u_r, v_r) for ``u [rows, K]`` and ``v [rows, N]``: (tile nodes ``[tiles, K, N]``, root
    ``[K, N]``).  A chunk of 64 rows is an fma chain from +0.0 over r ascending; rows past the end are absent."""
    rows, K, N = u.shape[0], u.shape[1], v.shape[1]
    chunks = -(-rows // CHUNK)
    up = np.zeros((chunks * CHUNK, K), dtype=np.float32)
    vp = np.zeros((chunks * CHUNK, N), dtype=np.float32)
    up[:rows], vp[:rows] = u, v
    up, vp = up.reshape(chunks, CHUNK, K), vp.reshape(chunks, CHUNK, N)
    acc = np.zeros((chunks, K, N), dtype=np.float32)
    for i in range(CHUNK):
        nxt = fma32(up[:, i, :, None], vp[:, i, None, :], acc)
        present = (np.arange(chunks) * CHUNK + i < rows)[:, None, None]
        acc = np.where(present, nxt, acc)
    tiles = tree32(acc, levels=2) if chunks % 4 == 0 else _tiles_of(acc)
    return tiles, tree32(tiles)[0]


def _tiles_of(chunk_nodes: np.ndarray) -> np.ndarray:
    """Two levels inside every tile of four chunks, the last tile holding fewer."""
    out = [tree32(chunk_nodes[c:c + 4])[0] for c in range(0, chunk_nodes.shape[0], 4)]
    return np.stack(out, axis=0)


def policy_net_reference(theta, obs, *, hidden: Sequence[int], n_modes: int, activation: str = "tanh", index=None,
                         grad_params=None, grad_value=None) -> Dict[str, np.ndarray]:
    """The definition of `wedm_policy_net` (include/wedm_hip.h) on host data.

    ``theta``: float32 ``[n_theta]``; ``obs``: float32 ``[n_src, D]``; ``index``: int64 ``[rows]`` or None (``rows ==
    n_src``).  Returns ``params`` (float32 ``[rows, P]``), ``value`` (``[rows]``) and the intermediates ``x``, ``a1``,
    ``h1``, ``a2``, ``h2``, ``out``; with ``grad_params`` (float32 ``[rows, >= P]``) and ``grad_value`` (``[rows]``) also ``grad_theta``
    (float32 ``[n_theta]``), ``partials`` (``[tiles, n_theta]``) and ``go``, ``da2``, ``da1``.  Nothing passed in is modified."""
    th, o = _host(theta).reshape(-1), _host(obs)
    if th.dtype != np.float32 or o.dtype != np.float32 or o.ndim != 2:
        raise ValueError("policy net: theta must be float32 [n_theta] and obs float32 [n_src, D]")
    n_src, D = o.shape
    check_dims(D, hidden, n_modes, activation)
    lay = layout(D, hidden, n_modes)
    if th.shape[0] != lay["n_theta"][0]:
        raise ValueError(f"policy net: theta holds {th.shape[0]} entries, the dims ask for {lay['n_theta'][0]}")
    W1, b1, W2, b2, W3, b3 = (th[at:at + int(np.prod(shape))].reshape(shape) for at, shape in (lay[k] for k in
                                                                                                ("W1", "b1", "W2", "b2", "W3", "b3")))
    P = 8 + int(n_modes)
    src = np.arange(n_src, dtype=np.int64) if index is None else _host(index).reshape(-1).astype(np.int64)
    rows = src.shape[0]
    if rows < 1 or rows > MAX_ROWS:
        raise ValueError(f"policy net: a call holds 1 to {MAX_ROWS} rows, got {rows}")
    bad = (src < 0) | (src >= n_src)
    x = np.where(bad[:, None], np.float32(0.0), clean32(o[np.where(bad, 0, src)])).astype(np.float32)
    a1 = layer32(x, W1, b1)
    h1 = _act(a1, activation)
    a2 = layer32(h1, W2, b2)
    h2 = _act(a2, activation)
    out = layer32(h2, W3, b3)
    res = {"params": _canon(out[:, :P]), "value": _canon(out[:, P]), "x": x, "a1": a1, "h1": h1, "a2": a2, "h2": h2, "out": out}
    if grad_params is None and grad_value is None:
        return res
    gp, gv = _host(grad_params), _host(grad_value).reshape(-1)
    if gp.dtype != np.float32 or gp.ndim != 2 or gp.shape[0] != rows or gp.shape[1] < P or gv.dtype != np.float32 or gv.shape != (rows,):
        raise ValueError(f"policy net: grad_params must be float32 [{rows}, >= {P}] and grad_value float32 [{rows}]")
    go = np.concatenate([gp[:, :P], gv[:, None]], axis=1).astype(np.float32)
    go = np.where(bad[:, None], np.float32(0.0), go).astype(np.float32)
    ones = np.ones((rows, 1), dtype=np.float32)
    with np.errstate(all="ignore"):
        da2 = (back32(go, W3) * _dact(h2, activation)).astype(np.float32)
        da1 = (back32(da2, W2) * _dact(h1, activation)).astype(np.float32)
    tiles_all, root_all = [], []
    for inp, g in ((x, da1), (h1, da2), (h2, go)):   # W | b per layer, the bias as the row of ones under the input
        t, r = rowsum32(np.concatenate([inp, ones], axis=1), g)
        tiles_all.append(t.reshape(t.shape[0], -1))
        root_all.append(r.reshape(-1))
    res.update(grad_theta=_canon(np.concatenate(root_all)), partials=_canon(np.concatenate(tiles_all, axis=1)), go=go, da2=da2, da1=da1)
    return res


class _Net(torch.autograd.Function):
    """(params, value) of the rows; the backward runs BACKWARD and FOLD into ``theta.grad`` itself and hands autograd
    nothing for ``theta``."""

    @staticmethod
    def forward(ctx, theta, net, obs, index):
        ctx.net, ctx.obs, ctx.index = net, obs, index
        ctx.set_materialize_grads(False)  # an output without a gradient arrives as None: `_backward` has cached zeros for it
        return net._forward(obs, index)

    @staticmethod
    def backward(ctx, gp, gv):
        ctx.net._backward(ctx.obs, ctx.index, gp, gv)
        return None, None, None, None


class PolicyNet:
    """``PolicyNet(vec_or_obs_dim, head, hidden=(64, 64), activation="tanh", seed=0, device=None)``: the actor-critic MLP
    between the observation and ``head``'s parameter row (a `PolicyHead`) plus a value estimate.

    ``theta`` is one flat float32 leaf with ``requires_grad`` (``W1, b1, W2, b2, W3, b3`` are views of it), drawn on the
    host from a seeded CPU generator, so it holds the same bits wherever the network lives.  ``forward(obs)`` returns
    ``(params [N, P], value [N])`` without a graph (``obs`` may be wider than ``obs_dim``: the leading ``obs_dim`` columns are
    read in place through the row stride, which is how an actor on the measured columns of a `Sensor` shares the critic's
    store); ``net(obs)`` and ``net(rollout=buf, index=idx)`` return the same with a
    graph whose backward writes ``theta.grad`` (adding to it where it exists).  The outputs are the network's own buffers,
    rewritten by its next call.  On a CPU device every call runs `policy_net_reference`.  After the first call of each
    shape nothing is allocated and nothing synchronises with the host."""

    def __init__(self, vec_or_obs_dim, head, hidden: Sequence[int] = (64, 64), activation: str = "tanh", seed: int = 0, device=None):
        D = int(vec_or_obs_dim) if isinstance(vec_or_obs_dim, (int, np.integer)) else len(vec_or_obs_dim.obs_names)
        self.head, self.obs_dim, self.hidden, self.activation = head, D, tuple(int(h) for h in hidden), str(activation)
        self.n_modes, self.param_dim = len(head.modes), head.param_dim
        check_dims(D, self.hidden, self.n_modes, self.activation)
        self.device = torch.device(head.device if device is None else device)
        native = getattr(head, "_native", None)
        self._native = native if self.device.type == "cuda" and hasattr(native, "policy_net") else None
        if self.device.type == "cuda" and self._native is None:
            raise ValueError("PolicyNet on a GPU needs a head whose backend has wedm_policy_net")
        self.layout = layout(D, self.hidden, self.n_modes)
        self.n_theta = self.layout["n_theta"][0]
        gen = torch.Generator().manual_seed(int(seed))
        th = torch.zeros(self.n_theta, dtype=torch.float32)
        for name, fan_in, gain in (("W1", D, 1.0), ("W2", self.hidden[0], 1.0), ("W3", self.hidden[1], 0.01)):
            at, shape = self.layout[name]
            n = shape[0] * shape[1]
            th[at:at + n] = torch.randn(n, generator=gen, dtype=torch.float32) * (gain / float(fan_in) ** 0.5)
        self.theta = th.to(self.device).requires_grad_(True)
        self._grad = torch.zeros(self.n_theta, dtype=torch.float32, device=self.device)
        self._params = torch.zeros((0, self.param_dim), dtype=torch.float32, device=self.device)
        self._value = torch.zeros(0, dtype=torch.float32, device=self.device)
        self._partials = torch.zeros((0, self.n_theta), dtype=torch.float32, device=self.device)
        self._zero_gv = torch.zeros(0, dtype=torch.float32, device=self.device)
        self._zero_gp = torch.zeros((0, self.param_dim), dtype=torch.float32, device=self.device)
        self._keep = None  # the inputs of the launches in flight

    def __getattr__(self, name: str) -> torch.Tensor:
        lay = self.__dict__.get("layout", {})
        if name in lay and name != "n_theta":
            at, shape = lay[name]
            return self.theta.detach()[at:at + int(np.prod(shape))].view(shape)
        raise AttributeError(name)

    # ------------------------------------------------------------------ arguments
    def _rows(self, obs, rollout, index):
        """(observation block ``[n_src, D]``, index or None, rows)."""
        if rollout is not None:
            if obs is not None or index is None:
                raise ValueError("rollout= goes with index= and without obs")
            obs = rollout.flat()["obs"]
        elif index is not None:
            raise ValueError("index= goes with rollout=")
        if not torch.is_tensor(obs) or obs.dtype != torch.float32 or obs.ndim != 2 or obs.shape[1] < self.obs_dim or obs.shape[0] < 1:
            raise ValueError(f"obs must be a float32 tensor [rows, >= {self.obs_dim}], got {getattr(obs, 'dtype', type(obs).__name__)} "
                             f"{list(getattr(obs, 'shape', []))}")
        if obs.device.type != self.device.type or (self.device.index is not None and obs.device.index != self.device.index):
            raise ValueError(f"obs lies on {obs.device}, the network on {self.device}")
        obs = obs.detach()[:, : self.obs_dim]  # a wider store: the leading columns, read in place through the row stride
        if obs.stride(1) != 1 or obs.stride(0) < self.obs_dim:
            obs = obs.contiguous()
        if index is not None:
            if not torch.is_tensor(index) or index.dtype != torch.int64 or index.ndim != 1 or index.shape[0] < 1 or index.device != obs.device:
                raise ValueError("index must be an int64 tensor [rows] on the observations' device")
            index = index.detach().contiguous()
        rows = obs.shape[0] if index is None else index.shape[0]
        if rows > MAX_ROWS:
            raise ValueError(f"a call holds at most {MAX_ROWS} rows ({_abi.NORM_MAX_TILES} tiles of {TILE}), got {rows}")
        return obs, index, rows

    def _desc(self, obs, index, rows: int, flags: int, **kw) -> "_abi.NetDesc":
        return _abi.NetDesc(theta=self.theta.data_ptr(), obs=obs.data_ptr(), index=None if index is None else index.data_ptr(),
                            obs_stride=obs.stride(0), n_src=obs.shape[0], obs_dim=self.obs_dim, hidden1=self.hidden[0],
                            hidden2=self.hidden[1], n_modes=self.n_modes, activation=ACTIVATIONS.index(self.activation), rows=rows,
                            param_stride=self.param_dim, grad_stride=self.param_dim, flags=flags, **kw)

    # ------------------------------------------------------------------ the calls
    def _forward(self, obs, index):
        rows = obs.shape[0] if index is None else index.shape[0]
        if self._params.shape[0] < rows:
            self._params = torch.zeros((rows, self.param_dim), dtype=torch.float32, device=self.device)
            self._value = torch.zeros(rows, dtype=torch.float32, device=self.device)
        params, value = self._params[:rows], self._value[:rows]
        if self._native is not None:
            d = self._desc(obs, index, rows, _abi.NET_FORWARD, params=params.data_ptr(), value=value.data_ptr())
            with torch.cuda.device(self.device):
                self._native.policy_net(d)
            self._keep = (obs, index)
        else:
            res = policy_net_reference(self.theta, obs, hidden=self.hidden, n_modes=self.n_modes, activation=self.activation, index=index)
            params.copy_(torch.from_numpy(res["params"]))
            value.copy_(torch.from_numpy(res["value"]))
        return params, value

    def _backward(self, obs, index, gp, gv) -> None:
        rows, P = obs.shape[0] if index is None else index.shape[0], self.param_dim
        if gv is None:
            if self._zero_gv.shape[0] < rows:
                self._zero_gv = torch.zeros(rows, dtype=torch.float32, device=self.device)
            gv = self._zero_gv[:rows]
        if gp is None:  # (only the value has a gradient: a critic)
            if self._zero_gp.shape[0] < rows:
                self._zero_gp = torch.zeros((rows, P), dtype=torch.float32, device=self.device)
            gp = self._zero_gp[:rows]
        gp, gv = gp.detach(), gv.detach().contiguous()
        if gp.stride(1) != 1 or gp.stride(0) < P:
            gp = gp.contiguous()
        tiles = -(-rows // TILE)
        if self._partials.shape[0] < tiles:
            self._partials = torch.zeros((tiles, self.n_theta), dtype=torch.float32, device=self.device)
        theta = self.theta
        fresh = theta.grad is None
        target = self._grad if fresh else theta.grad
        if self._native is not None:
            flags = _abi.NET_BACKWARD | _abi.NET_FOLD | (0 if fresh else _abi.NET_ACCUMULATE)
            d = self._desc(obs, index, rows, flags, grad_params=gp.data_ptr(), grad_value=gv.data_ptr(),
                           partials=self._partials.data_ptr(), grad_theta=target.data_ptr())
            d.grad_stride = gp.stride(0)
            with torch.cuda.device(self.device):
                self._native.policy_net(d)
            self._keep = (obs, index, gp, gv)
        else:
            res = policy_net_reference(theta, obs, hidden=self.hidden, n_modes=self.n_modes, activation=self.activation, index=index,
                                       grad_params=gp, grad_value=gv)
            self._partials[:tiles].copy_(torch.from_numpy(res["partials"]))
            g = res["grad_theta"]
            if not fresh:
                with np.errstate(all="ignore"):
                    g = _canon(_host(target) + g)
            target.copy_(torch.from_numpy(g))
        if fresh:
            theta.grad = target

    def forward(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(params [N, P], value [N])`` of ``obs`` (float32 ``[N, D]``) without a graph: one launch."""
        obs, index, _ = self._rows(obs, None, None)
        return self._forward(obs, index)

    def __call__(self, obs: Optional[torch.Tensor] = None, *, rollout=None, index: Optional[torch.Tensor] = None):
        """``(params, value)`` with a graph: of ``obs`` (float32 ``[B, D]``), or of the steps ``index`` (int64 ``[B]``) of
        ``rollout``'s observation block, read in place.  The backward recomputes the activations from the same block, which
        must hold until then, and writes ``theta.grad``: into the network's own gradient buffer where it was None, else
        added to it with one float32 addition per element."""
        obs, index, _ = self._rows(obs, rollout, index)
        params, value = _Net.apply(self.theta, self, obs, index)
        return params, value

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        return {"theta": self.theta.detach().cpu().clone(), "obs_dim": self.obs_dim, "hidden": list(self.hidden),
                "n_modes": self.n_modes, "activation": self.activation}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Refuses other dims or another activation and then leaves every byte as it was."""
        mine = (self.obs_dim, list(self.hidden), self.n_modes, self.activation)
        theirs = (int(sd["obs_dim"]), [int(h) for h in sd["hidden"]], int(sd["n_modes"]), str(sd["activation"]))
        if mine != theirs:
            raise ValueError(f"PolicyNet: the dict was written by a network of dims (obs_dim, hidden, n_modes, activation) = {theirs}, "
                             f"this one has {mine}")
        th = sd["theta"]
        if not torch.is_tensor(th) or th.dtype != torch.float32 or tuple(th.shape) != (self.n_theta,):
            raise ValueError(f"PolicyNet: theta must be a float32 tensor [{self.n_theta}]")
        with torch.no_grad():
            self.theta.copy_(th)
