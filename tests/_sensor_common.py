"""What tests/test_sensor_host.py (the definition and the adapter, on the host) and tests/test_sensor.py (the kernel against
the definition, on the MI355X) share: problems of `wedm_sensor` laid out in ONE byte arena -- every block between guard bands,
padding columns behind every struct-of-arrays row -- so that "every byte the call may write, and no other" is one comparison
of two buffers; channel tables by kind; the sequence of calls with restarts and masked environments; sensors, environments
and the asymmetric training stack (an actor on the measured columns, a critic on all of them).  TEST SEAM ONLY."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from sparc_amd import (Adam, Channel, EpisodeLog, Normalizer, PolicyHead, PolicyNet, PPOLoss, RolloutBuffer, Sensor,
                       WireEDMVectorEnv, _abi)
from sparc_amd.sensor import sensor_reference
from tests import _policy_net_common as pc
from tests import _resume_common as rc
from tests._episode_log_common import FILL, GUARD, NAN32, differences  # noqa: F401  (differences: re-exported)
from tests._reward_common import every_term, shaped_env

SN = _abi.SN
KINDS = ("all", "identity", "sigma", "calib", "delay", "lsb", "clamp", "mixed")
WRAP = 2 ** 32 - 3   # an env_id_offset at which the global id wraps inside the batch
SEED = 0xFEDC_BA98_7654_3210
T0 = 2 ** 32 - 5     # the first call number: the sequence crosses 2^32
K0 = 2 ** 32 - 2     # the first episode numbers: some cross 2^32 at once
CALLS = 12


def channel_table(rng, C_in: int, C_out: int, L: int, kind: str) -> Tuple[np.ndarray, np.ndarray]:
    """(chan ``[6, C_out]``, route ``[2, C_out]``) with the stages ``kind`` names switched on: every one, none, one alone, or
    a random subset per channel."""
    chan = np.zeros((_abi.SENSOR_FIELDS, C_out))
    chan[SN.LO], chan[SN.HI] = -np.inf, np.inf
    route = np.zeros((_abi.SENSOR_ROUTES, C_out), dtype=np.int32)
    route[_abi.SN_SOURCE] = rng.integers(0, C_in, C_out)
    for c in range(C_out):
        on = {"all": KINDS[2:7], "identity": (), "mixed": tuple(k for k in KINDS[2:7] if rng.random() < 0.5)}.get(kind, (kind,))
        if "sigma" in on:
            chan[SN.SIGMA, c] = rng.uniform(0.01, 2.0)
        if "calib" in on:
            chan[SN.GAIN_SPREAD, c], chan[SN.OFFSET_SPREAD, c] = rng.uniform(0.01, 0.2), rng.uniform(0.1, 1.0)
        if "delay" in on:
            route[_abi.SN_MAX_DELAY, c] = L - 1 if c == 0 else rng.integers(0, L)
        if "lsb" in on:
            chan[SN.LSB, c] = (0.25, 0.1, 1.0 / 3.0)[c % 3]
        if "clamp" in on:
            chan[SN.LO, c], chan[SN.HI, c] = -4.0, 6.5
    return chan, route


class Problem:
    """One set of blocks for `wedm_sensor` in one arena.  ``planes``: rows per source plane; ``pad``: columns past
    ``num_envs`` in the planes, ``out`` and the ring (each its own: pad, pad + 1, pad + 2 where pad > 0).  ``pos`` and ``age``
    start as garbage: the first call marks every environment as starting an episode."""

    def __init__(self, rng, N: int, planes: Sequence[int] = (8,), C_out: int = 5, L: int = 2, kind: str = "all", pad: int = 3,
                 offset: int = 0, table: Optional[Tuple[np.ndarray, np.ndarray]] = None):
        self.N, self.rows, self.C_in, self.C_out, self.L, self.offset = int(N), tuple(planes), sum(planes), int(C_out), int(L), int(offset)
        self.S, self.OS, self.RS = N + pad, N + (pad + 1 if pad else 0), N + (pad + 2 if pad else 0)
        self.layout: Dict[str, Tuple[int, np.dtype, tuple]] = {}
        self._init: Dict[str, np.ndarray] = {}
        self._size = GUARD
        chan, route = channel_table(rng, self.C_in, C_out, L, kind) if table is None else table
        for k, r in enumerate(self.rows):
            self._add(f"plane{k}", (rng.standard_normal((r, self.S)) * 10.0).astype(np.float32))
        self._add("chan", chan)
        self._add("route", route.astype(np.int32))
        self._add("first", np.ones(N, dtype=np.uint8))
        self._add("mask", np.ones(N, dtype=np.uint8))
        self._add("episode", (K0 + np.arange(N) % 4).astype(np.int64))
        self._add("out", (rng.standard_normal((C_out, self.OS)) * 7.0).astype(np.float32))
        if L > 1:
            self._add("ring", (rng.standard_normal((L, self.C_in, self.RS)) * 7.0).astype(np.float32))
        info = np.iinfo(np.int32)
        garbage = np.array([info.min, info.max, -1, 0, 1, 7, 8, 1 << 20], dtype=np.int32)
        self._add("pos", garbage[rng.integers(0, garbage.size, N)])
        self._add("age", garbage[rng.integers(0, garbage.size, N)])
        self.buf = np.full(self._size, FILL, dtype=np.uint8)
        for name, a in self._init.items():
            self.view(self.buf, name)[...] = a
        del self._init

    def _add(self, name: str, a: np.ndarray) -> None:
        off = -(-self._size // 16) * 16
        self.layout[name] = (off, a.dtype, a.shape)
        self._init[name] = a
        self._size = off + a.nbytes + GUARD

    def view(self, buf: np.ndarray, name: str) -> np.ndarray:
        off, dt, shape = self.layout[name]
        return buf[off: off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

    def define(self, buf: np.ndarray, t: int, part: Optional[Tuple[int, int]] = None, first: bool = True, mask: bool = True,
               episode: bool = True, trace: Optional[dict] = None) -> None:
        """`sensor_reference` on the blocks of ``buf``, in place.  ``part = (begin, count)``: the shard of that many
        environments from ``begin`` on; ``first`` / ``mask`` / ``episode``: whether the block is passed or None."""
        b, n = part or (0, self.N)
        v = lambda name: self.view(buf, name)   # noqa: E731
        sensor_reference([v(f"plane{k}")[:, b:] for k in range(len(self.rows))], v("chan"), v("route"),
                         v("first")[b: b + n] if first else None, v("mask")[b: b + n] if mask else None,
                         v("episode")[b: b + n] if episode else None, v("out")[:, b:], v("ring")[:, :, b:] if self.L > 1 else None,
                         v("pos")[b: b + n], v("age")[b: b + n], seed=SEED, t=t, env_id_offset=(self.offset + b) & 0xFFFFFFFF,
                         num_envs=n, ring_len=self.L, trace=trace)

    def desc(self, base: int, t: int, part: Optional[Tuple[int, int]] = None, first: bool = True, mask: bool = True,
             episode: bool = True) -> "_abi.SensorDesc":
        """The descriptor of the same call on a copy of the arena at address ``base``."""
        b, n = part or (0, self.N)
        at = lambda name: base + self.layout[name][0] + b * self.layout[name][1].itemsize   # noqa: E731
        d = _abi.SensorDesc(chan=base + self.layout["chan"][0], route=base + self.layout["route"][0],
                            first=at("first") if first else None, mask=at("mask") if mask else None,
                            episode=at("episode") if episode else None, out=at("out"), ring=at("ring") if self.L > 1 else None,
                            pos=at("pos"), age=at("age"), out_stride=self.OS, ring_stride=self.RS if self.L > 1 else 0, seed=SEED, t=t,
                            env_id_offset=(self.offset + b) & 0xFFFFFFFF, num_envs=n, n_out=self.C_out, ring_len=self.L)
        for k, r in enumerate(self.rows):
            d.plane[k].rows, d.plane[k].n_rows, d.plane[k].stride = at(f"plane{k}"), r, self.S
        return d


def sequence_inputs(p: Problem, rng, call: int) -> Dict[str, np.ndarray]:
    """The inputs of call ``call`` of the twelve: fresh sources; every environment starts at call 0; environment e with
    e % 3 == 0 restarts (with the next episode number) at call 3 + (e // 3) % 7; environments with e % 5 == 1 are masked out
    in calls 4 to 6.  Returns {block name: new contents}."""
    N, e = p.N, np.arange(p.N)
    new = {f"plane{k}": (rng.standard_normal((r, p.S)) * 10.0).astype(np.float32) for k, r in enumerate(p.rows)}
    restart = (e % 3 == 0) & (call == 3 + (e // 3) % 7)
    new["first"] = np.where((call == 0) | restart, rng.integers(1, 256, N), 0).astype(np.uint8)
    new["mask"] = np.where((e % 5 == 1) & (4 <= call <= 6), 0, rng.integers(1, 256, N)).astype(np.uint8)
    restarts_so_far = ((e % 3 == 0) & (call >= 3 + (e // 3) % 7)).astype(np.int64)
    new["episode"] = (K0 + e % 4 + restarts_so_far).astype(np.int64)
    return new


def hostile_f32(rng, shape) -> np.ndarray:
    """NaNs with payloads, both infinities, subnormals, both zeros, FLT_MAX and ordinary values, shuffled."""
    fmax = np.finfo(np.float32).max
    pool = np.array([NAN32[0], NAN32[1], np.inf, -np.inf, 1e-45, -1e-45, 5e-39, -0.0, 0.0, fmax, -fmax, 1.0, -3.5, 0.125, 7.25],
                    dtype=np.float32)
    pool[:2] = NAN32
    return pool[rng.integers(0, pool.size, shape)]


def hostile_table(rng, C_in: int, C_out: int, L: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per channel one of: identity; ``lsb`` 1e-300; ``lsb`` 1e300; ``sigma`` 1e300; every stage at ordinary values; a
    negative ``lsb`` (off) with ``lo > hi``; and ``SOURCE`` / ``MAX_DELAY`` entries far outside their ranges throughout."""
    chan, route = channel_table(rng, C_in, C_out, L, "identity")
    usual = channel_table(rng, C_in, C_out, L, "all")[0]
    info = np.iinfo(np.int32)
    for c in range(C_out):
        how = c % 6
        if how == 1:
            chan[SN.LSB, c] = 1e-300
        elif how == 2:
            chan[SN.LSB, c] = 1e300
        elif how == 3:
            chan[SN.SIGMA, c] = 1e300
        elif how == 4:
            chan[:, c] = usual[:, c]
        elif how == 5:
            chan[SN.LSB, c], chan[SN.LO, c], chan[SN.HI, c] = -0.5, 2.0, -2.0
        route[_abi.SN_SOURCE, c] = (-5, 1000, info.min, info.max, 3, -1)[c % 6]
        route[_abi.SN_MAX_DELAY, c] = (info.max, -7, 1000, info.min, 1, 9)[(c // 2) % 6]
    return chan, route


# ------------------------------------------------------------------------------------------------ sensors and stacks
def noisy_sensor(raw: Sequence[str], seed: int = 5, privileged="all") -> Sensor:
    """Noise, calibration and delays of 0, 1 and 3 on some channels, quantisation and saturation on others; the measurable
    columns that ``raw`` holds, and the first wire-profile column where there is one."""
    from sparc_amd.sensor import MEASURABLE_OBS_NAMES

    have = [n for n in MEASURABLE_OBS_NAMES if n in raw]
    spec = {"wire_velocity": dict(sigma=0.02, max_delay=1), "voltage": dict(sigma=0.5, gain_spread=0.02, offset_spread=0.3, lsb=0.25,
                                                                           lo=0.0, hi=200.0, max_delay=3),
            "current": dict(sigma=0.3, gain_spread=0.05, lsb=0.125, max_delay=1), "spark_state": dict(),
            "spark_pulses": dict(max_delay=3), "short_pulses": dict(offset_spread=0.5, lsb=1.0), "short_steps": dict(sigma=1.0, lo=0.0),
            "current_sum": dict(gain_spread=0.03), "energy_sum": dict(sigma=5.0, gain_spread=0.03, max_delay=1)}
    channels = [Channel(n, **spec[n]) for n in have]
    if "wire_zone_mean" in raw:
        channels.append(Channel("wire_zone_mean", name="pyrometer", sigma=2.0, offset_spread=5.0, lsb=0.5, max_delay=3))
    return Sensor(channels, privileged=privileged, seed=seed)


def in_kernel_stack(device: str, capacity: int = 256, n: int = 64):
    """64 x 13, in-kernel autoreset, pulse and signal columns, the wire profile, `noisy_sensor`, a `Normalizer`, the
    `ShapedReward` of `tests._reward_common.every_term` and an `EpisodeLog`, reset and put into
    `tests._snapshot_common.scenario`.  Returns (vec, log, action)."""
    from tests import _snapshot_common as snap
    from sparc_amd.profile import profile_names

    env = shaped_env(device, n)
    log = EpisodeLog(capacity=capacity)
    raw = tuple(env.obs_names) + profile_names(2)
    vec = WireEDMVectorEnv(env, max_episode_steps=3000, wire_profile_bins=2, reward=every_term(), sensor=noisy_sensor(raw),
                           normalizer=Normalizer(gamma=0.9, clip_obs=5.0), episode_log=log)
    vec.reset(seed=33)
    return vec, log, snap.scenario(env, seed=77)


def sensor_blocks(s: Sensor) -> Dict[str, torch.Tensor]:
    """Host copies of everything a bound `Sensor` holds."""
    sd = s.state_dict()
    out = {f"sensor.{k}": sd[k] for k in ("out", "pos", "age")}
    if sd["ring"] is not None:
        out["sensor.ring"] = sd["ring"]
    out["sensor.seed_t"] = torch.from_numpy(np.array([sd["seed"], sd["t"]], dtype=np.uint64).view(np.int64).copy())
    return out


def _patched_vector_env(seed: int):
    """`WireEDMVectorEnv` with a `noisy_sensor` added to whatever `tests._resume_common.Stack` passes."""
    from sparc_amd.profile import profile_names

    def make(env, **kw):
        raw = tuple(env.obs_names) + (profile_names(kw["wire_profile_bins"]) if kw.get("wire_profile_bins") is not None else ())
        return WireEDMVectorEnv(env, sensor=noisy_sensor(raw, seed=seed), **kw)

    return make


def sensor_stack(variant: str, device: str, seeds: dict, cls=None) -> rc.Stack:
    """The stack ``variant`` of tests/_resume_common.py built with a sensor: `tests._resume_common.Stack` is constructed
    while its module's ``WireEDMVectorEnv`` name is bound to `_patched_vector_env`."""
    keep = rc.WireEDMVectorEnv
    rc.WireEDMVectorEnv = _patched_vector_env(seeds["head"] + 1000)
    try:
        return (cls or rc.Stack)(variant, device, seeds)
    finally:
        rc.WireEDMVectorEnv = keep


def stack_everything(st) -> Dict[str, torch.Tensor]:
    out = rc.everything(st)
    out.update(sensor_blocks(st.vec.sensor))
    return out


def check_resume_at_every_cut(variant: str, device: str, folder) -> None:
    """Cut after every control step, saved, loaded into a fresh stack built with other seeds (its sensor's included) and
    dirtied, continued: everything handed out and held afterwards equals the uninterrupted run's on every byte."""
    st = sensor_stack(variant, device, rc.RUN_SEEDS)
    steps: List[dict] = []
    calls: List[dict] = []
    paths = []
    for k in rc.CUTS:
        rc.run(st, k, steps, calls)
        paths.append(folder / f"sensor-{variant}-{k}.pt")
        rc.save(st, paths[-1])
    rc.run(st, rc.K, steps, calls)
    end = stack_everything(st)
    noisy = torch.stack([s["obs"] for s in steps])
    st.close()
    assert len(calls) == 4 and len(set(noisy.reshape(-1).tolist())) > 64
    for k in rc.CUTS:
        other = sensor_stack(variant, device, rc.OTHER_SEEDS)
        try:
            rc.run(other, 2, [], [])
            rc.load(other, paths[k])
            got_steps, got_calls = [], []
            rc.run(other, rc.K, got_steps, got_calls)
            for i, (got, want) in enumerate(zip(got_steps, steps[k:])):
                rc.assert_equal(got, want, f"{variant}, cut {k}: what control step {k + i + 1} handed out")
            want_calls = [c for c in calls if c["step"] >= k]
            for got, want in zip(got_calls, want_calls):
                rc.assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, f"{variant}, cut {k}")
            rc.assert_equal(stack_everything(other), end, f"{variant}, cut {k}: everything after control step {rc.K}")
        finally:
            other.close()


# ------------------------------------------------------------------------------------------------ the asymmetric run
class AsymmetricStack:
    """64 x 13, in-kernel autoreset: an actor `PolicyNet` on the sensor's ``actor_dim`` measured columns and a critic
    `PolicyNet` on all columns, both reading the rollout's observation block in place, `PPOLoss.backward(rollout=, index=)`,
    two `Adam`s."""

    def __init__(self, device: str, seeds: dict):
        from tests import _snapshot_common as snap
        from sparc_amd.profile import profile_names

        self.device = device
        self.env = shaped_env(device, 64)
        raw = tuple(self.env.obs_names) + profile_names(2)
        self.sensor = noisy_sensor(raw, seed=seeds["head"] + 1000)
        self.norm = Normalizer(gamma=0.9, clip_obs=5.0)
        self.vec = vec = WireEDMVectorEnv(self.env, max_episode_steps=3000, wire_profile_bins=2, reward=every_term(),
                                          sensor=self.sensor, normalizer=self.norm)
        self.head = PolicyHead(vec, modes=rc.MODES, bounds=rc.BOUNDS, seed=seeds["head"])
        self.ppo = PPOLoss(self.head, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
        self.buf = RolloutBuffer(vec, rc.T, gamma=0.95, extras={"log_prob": torch.float32})
        self.actor = PolicyNet(vec.actor_obs_dim, self.head, hidden=pc.NET_HIDDEN, seed=seeds["net"])
        self.critic = PolicyNet(vec, self.head, hidden=pc.NET_HIDDEN, seed=seeds["net"] + 1)
        self.opts = [Adam(self.actor, lr=1e-2, max_grad_norm=0.5), Adam(self.critic, lr=2e-2, max_grad_norm=0.5)]
        self.steps, self.pending = 0, False
        obs, _ = vec.reset(seed=seeds["reset"])
        snap.scenario(self.env, seed=seeds["scenario"])
        self.buf.reset()
        self.obs = obs.clone()

    def epoch(self) -> None:
        rows = rc.T * self.vec.num_envs
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1000 + self.steps)).to(self.device)
        for opt in self.opts:
            opt.begin_update()
        for idx in torch.tensor_split(perm, 2):
            for opt in self.opts:
                opt.zero_grad()
            params, _ = self.actor(rollout=self.buf, index=idx)
            _, value = self.critic(rollout=self.buf, index=idx)
            self.ppo.backward(params, value, rollout=self.buf, index=idx)
            for opt in self.opts:
                opt.step(None)
        for opt in self.opts:
            opt.zero_grad()

    def run(self, upto: int) -> None:
        while self.steps < upto:
            if self.pending:
                self.epoch()
                self.pending = False
            with torch.no_grad():
                params = self.actor.forward(self.obs)[0].clone()
                value = self.critic.forward(self.obs)[1].clone()
                out = self.head.sample(params)
                nxt, reward, term, trunc, _ = self.vec.step(out.action)
                self.buf.add(self.obs, self.head.stored(out), value, reward, term, trunc, log_prob=out.log_prob)
                self.obs = nxt.clone()
                self.steps += 1
                if self.steps % rc.T == 0:
                    self.buf.finish(self.critic.forward(self.obs)[1].clone())
                    self.pending = True
        self.env.check_errors()

    def everything(self) -> Dict[str, torch.Tensor]:
        host = lambda t: t.detach().cpu().clone()   # noqa: E731
        out = {"actor.theta": host(self.actor.theta), "critic.theta": host(self.critic.theta), "loop.obs": host(self.obs)}
        for name, opt in zip(("actor", "critic"), self.opts):
            out.update({f"{name}.m": host(opt.m), f"{name}.v": host(opt.v), f"{name}.state": host(opt.state)})
        out.update(sensor_blocks(self.sensor))
        out["norm.stats"] = host(self.norm.stats)
        return out

    def save(self, path) -> None:
        torch.save({"vec": self.vec.state_dict(), "head": self.head.state_dict(), "buf": self.buf.state_dict(),
                    "ppo": self.ppo.state_dict(), "actor": self.actor.state_dict(), "critic": self.critic.state_dict(),
                    "opts": [o.state_dict() for o in self.opts], "steps": self.steps, "pending": self.pending,
                    "obs": self.obs.detach().cpu().clone()}, path)

    def load(self, path) -> None:
        ck = torch.load(path, map_location="cpu", weights_only=True)
        self.vec.load_state_dict(ck["vec"])
        self.head.load_state_dict(ck["head"])
        self.buf.load_state_dict(ck["buf"])
        self.ppo.load_state_dict(ck["ppo"])
        self.actor.load_state_dict(ck["actor"])
        self.critic.load_state_dict(ck["critic"])
        for o, sd in zip(self.opts, ck["opts"]):
            o.load_state_dict(sd)
        self.steps, self.pending, self.obs = int(ck["steps"]), bool(ck["pending"]), ck["obs"].to(self.device)

    def close(self) -> None:
        self.vec.close()
