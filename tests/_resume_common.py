"""What tests/test_resume_host.py (CPU oracle backends, the torch and NumPy paths) and tests/test_resume.py (MI355X, the
kernels) share: whole training stacks -- environment, vector adapter, episode sampler, normaliser, policy head, rollout
buffer, PPO loss and a small network -- by variant name, the loop that drives them, checkpoints of everything through
``torch.save``, resumes into fresh objects through the public calls, and byte-for-byte comparison of everything a run hands
out and holds.  TEST SEAM ONLY.

The loop.  Control step ``i`` (1-based): if an epoch is pending, run it (two minibatches through
``PPOLoss.backward(rollout=, index=)``, each moving the network by a fixed step); choose the actions with `PolicyHead.sample`
from the network's output at the current observation; ``vec.step``; ``buf.add``; after every ``T``-th step ``buf.finish`` and
mark the epoch pending.  A cut ``k`` lies after control step ``k``: cuts 1 .. 3 and 5 .. 7 inside a rollout, cuts 4 and 8
right after `finish` (slot 0, the new ``prev_done`` live) and before the epoch over that rollout, cut 0 before the first step.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from sparc_amd.ppo import STAT_NAMES
from sparc_amd import EnvironmentConfig, EpisodeSampler, Normalizer, PolicyHead, PPOLoss, RolloutBuffer, WireEDMEnv, WireEDMVectorEnv
from tests import _snapshot_common as snap
from tests._signal_oracle import SignalOracleBackend
from tests.test_episode_sampler import sampler_blocks
from tests.test_episode_sampler_host import DEFAULTS, DIAMETERS, HEIGHT, MATERIALS, RANGES, WIRE

T = 4                    # steps of a rollout
K = 2 * T + 1            # control steps of a run: two `finish` calls, two epochs, one step after the second
CUTS = tuple(range(K))
VARIANTS = ("in-kernel", "host-reset", "frozen")
MODES = (5, 9, 13)
BOUNDS = {"servo": (-0.2, 0.4), "ON_time": (1.0, 4.0), "OFF_time": (20.0, 60.0)}
HIDDEN = 32
LEARNING_RATE = 0.5
# (reset, scenario, sampler, head, network): the run's, and those a fresh stack is built and dirtied with
RUN_SEEDS = dict(reset=33, scenario=77, sampler=0x1234_5678_9ABC_DEF0, head=111, net=5)
OTHER_SEEDS = dict(reset=34, scenario=78, sampler=0x0FED_CBA9_8765_4321, head=112, net=6)


# ------------------------------------------------------------------------------------------------ environments
def episode_env(device: str, n: int = 70, offset: int = 3000, **kw) -> WireEDMEnv:
    """The environment of ``tests/test_episode_sampler.py::make`` (per-environment parameters, four materials, dynamic
    geometry) with the pulse and signal accumulators and a crater log of 8 added; on the CPU the oracle backend that keeps
    the signal rows."""
    kw.setdefault("config", EnvironmentConfig(target_cutting_distance=5000.0))
    if device == "cpu":
        kw["backend"] = SignalOracleBackend
    return WireEDMEnv(num_envs=n, device=device, wire_params=WIRE, env_id_offset=offset, env_params=dict(DEFAULTS),
                      workpiece_height=np.linspace(1.5, 9.5, n), wire_material=[MATERIALS[k % 4] for k in range(n)],
                      wire_material_table=MATERIALS[:4], dynamic_geometry={"max_workpiece_height": 10.0, "wire_diameters": DIAMETERS},
                      wire_diameter=np.resize(DIAMETERS, n), pulse_stats=True, signal_stats=True, crater_log_capacity=8, **kw)


def env_everything(env) -> Dict[str, torch.Tensor]:
    """`tests._snapshot_common.everything` and, where the geometry is per environment, its rows, heights and diameters.  The
    state blocks are whole, padding included.  The per-environment rows beside them (parameters, material, geometry) are cut
    to the batch: their padding columns are no state -- `set_wire_material`, which a load goes through, fills them with the
    last environment's entry, a draw of the episode sampler leaves them as they were."""
    out, n = dict(snap.everything(env)), env.num_envs
    if getattr(env, "per_env_geometry", False):
        out["_geom_f64"] = env._geom_f64.detach().cpu().clone()
        out["_geom_i32"] = env._geom_i32.detach().cpu().clone()
    if getattr(env, "_dyn", None) is not None:
        out["_dyn.height"] = env._dyn.height.detach().cpu().clone()
        out["_dyn.dia"] = env._dyn.dia.detach().cpu().clone()
    return {k: (v[..., :n].clone() if k.startswith("_") else v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ byte comparison
def _ne(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise: any byte differs (NaN payloads and signed zeros count)."""
    a, b = a.contiguous(), b.contiguous()
    size = a.element_size()
    ra = a.reshape(-1).view(torch.uint8).reshape(-1, size)
    rb = b.reshape(-1).view(torch.uint8).reshape(-1, size)
    return (ra != rb).any(dim=1).reshape(a.shape)


def first_difference(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> Optional[str]:
    """None, or the first block (in the order of ``want``) that differs in any byte, with the index of its first such
    element (for a per-environment block the last index is the environment)."""
    assert list(got) == list(want), (sorted(set(got) ^ set(want)))
    for name in want:
        a, b = got[name], want[name]
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{name}: {a.dtype} {list(a.shape)} against {b.dtype} {list(b.shape)}"
        if a.numel() == 0:
            continue
        bad = _ne(a, b)
        if bool(bad.any()):
            at = bad.reshape(bad.shape if bad.dim() else (1,)).nonzero()[0].tolist()
            return f"{name} at {at} ({int(bad.sum())} of {bad.numel()} elements differ)"
    return None


def assert_equal(got, want, where) -> None:
    bad = first_difference(got, want)
    assert bad is None, (where, bad)


# ------------------------------------------------------------------------------------------------ the stack
class Stack:
    """Everything one training process holds.  ``steps`` (control steps done), ``pending`` (an epoch is due) and ``obs`` (the
    observation the next action is chosen from) are the loop's own variables: a checkpoint carries them too."""

    def __init__(self, variant: str, device: str, seeds: dict, net_device: Optional[str] = None):
        self.variant, self.device, self.net_device = variant, device, net_device or device
        self.sampler = self.norm = None
        if variant == "in-kernel":
            self.env = snap.make(device, 64, "autoreset", "s13")
            self.norm = Normalizer(gamma=0.9, clip_obs=5.0)
            self.vec = WireEDMVectorEnv(self.env, max_episode_steps=3000, wire_profile_bins=2, normalizer=self.norm)
        elif variant == "host-reset":
            self.env = episode_env(device, 70)
            self.sampler = EpisodeSampler(seeds["sampler"], params=RANGES, materials=True, height=HEIGHT, diameters=True)
            self.vec = WireEDMVectorEnv(self.env, episode_sampler=self.sampler, max_episode_steps=2000, reward="progress")
        elif variant == "frozen":
            self.env = snap.make(device, 70, "all", "s13")
            self.norm = Normalizer(gamma=0.9, clip_obs=5.0)
            self.vec = WireEDMVectorEnv(self.env, autoreset=False, max_episode_steps=8000, reward="progress", normalizer=self.norm)
        else:
            raise KeyError(variant)
        vec = self.vec
        self.head = PolicyHead(vec, modes=MODES, bounds=BOUNDS, seed=seeds["head"])
        self.ppo = PPOLoss(self.head, clip=0.2, vf_coef=0.5, ent_coef=0.01, clip_value=0.3)
        self.buf = RolloutBuffer(vec, T, gamma=0.95, extras={"log_prob": torch.float32})
        gen = torch.Generator(device=self.net_device).manual_seed(seeds["net"])
        D, P = len(vec.obs_names), self.head.param_dim
        leaf = lambda *shape: (0.1 * torch.randn(*shape, generator=gen, device=self.net_device)).requires_grad_(True)   # noqa: E731
        self.leaves = [leaf(D, HIDDEN), leaf(HIDDEN), leaf(HIDDEN, P), leaf(P), leaf(HIDDEN, 1), leaf(1)]
        self.scale = 0.3 if self.norm is not None else 1e-3   # (raw observations hold volts and kelvins)
        self.steps, self.pending, self.obs = 0, False, None
        self._start(seeds)

    def _start(self, seeds: dict) -> None:
        """One reset through the adapter, then `tests._snapshot_common.scenario`: every tenth environment reaches its target
        at once, every tenth breaks its wire, every tenth ends in mid-interval.  With an episode sampler two masked resets
        come first, so that the draw counts differ from the start."""
        vec, n = self.vec, self.vec.num_envs
        obs, _ = vec.reset(seed=seeds["reset"])
        if self.sampler is not None:
            idx = torch.arange(n, device=self.env.device)
            for m in (3, 4):
                obs, _ = vec.reset(options={"mask": idx % m == 0})
        snap.scenario(self.env, seed=seeds["scenario"])
        self.buf.reset()
        self.obs = obs.clone()

    def net(self, obs: torch.Tensor):
        """(params, value) on the stack's device, from the two-layer network where it lives."""
        W1, b1, Wp, bp, Wv, bv = self.leaves
        x = torch.nan_to_num(obs).to(self.net_device) * self.scale
        h = torch.tanh(x @ W1 + b1)
        return (h @ Wp + bp).to(self.device), (h @ Wv + bv).squeeze(1).to(self.device)

    def close(self) -> None:
        self.vec.close()


def _host(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().clone()


def epoch(st: Stack, calls: List[dict]) -> None:
    """One epoch of two minibatches over the finished rollout; the permutation is a function of the step number."""
    flat = st.buf.flat()
    rows, P = T * st.vec.num_envs, st.head.param_dim
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1000 + st.steps)).to(st.device)
    for part, idx in enumerate(torch.tensor_split(perm, 2)):
        params, value = st.net(flat["obs"][idx])
        stats = st.ppo.backward(params, value, rollout=st.buf, index=idx)
        B = idx.shape[0]
        calls.append({"step": st.steps, "part": part, "grad": _host(st.ppo._grad[: B * (P + 1)]), "stats": _host(stats.tensor)})
        with torch.no_grad():
            for leaf in st.leaves:
                leaf -= LEARNING_RATE * leaf.grad
                leaf.grad = None


def control_step(st: Stack, steps: List[dict], calls: List[dict]) -> None:
    if st.pending:
        epoch(st, calls)
        st.pending = False
    with torch.no_grad():
        params, value = st.net(st.obs)
        out = st.head.sample(params)
        nxt, reward, term, trunc, info = st.vec.step(out.action)
        st.buf.add(st.obs, st.head.stored(out), value, reward, term, trunc, log_prob=out.log_prob)
        rec = {"obs": _host(nxt), "reward": _host(reward), "terminated": _host(term), "truncated": _host(trunc),
               "episode": _host(info["episode"])}
        if st.norm is not None:
            rec.update({f"episode_stats.{k}": _host(v) for k, v in info["episode_stats"].items()})
            rec.update(raw_observation=_host(info["raw_observation"]), raw_reward=_host(info["raw_reward"]))
        steps.append(rec)
        st.obs = nxt.clone()
        st.steps += 1
        if st.steps % T == 0:
            st.buf.finish(st.net(st.obs)[1])
            st.pending = True


def run(st: Stack, upto: int, steps: List[dict], calls: List[dict]) -> None:
    while st.steps < upto:
        control_step(st, steps, calls)
    st.env.check_errors()


def everything(st: Stack) -> Dict[str, torch.Tensor]:
    """Host copies of all a stack holds: the environment's blocks and rows, the sampler's, the normaliser's statistics and
    rows, the head's seed and step number, the buffer's state dict and (once a rollout was finished) `flat`, the adapter's
    own two tensors, the network's leaves and the loop's observation."""
    out = {f"env.{k}": v for k, v in env_everything(st.env).items()}
    if st.sampler is not None:
        out.update({f"sampler.{k}": v for k, v in sampler_blocks(st.env, st.sampler).items()})
    if st.norm is not None:
        out["norm.stats"] = _host(st.norm.stats)
        out.update({f"norm.rows.{k}": _host(v) for k, v in st.norm.rows.items()})
    out["head.seed_t"] = torch.from_numpy(np.array([st.head.seed, st.head.t], dtype=np.uint64).view(np.int64).copy())
    sd = st.buf.state_dict()
    out["buf.slot"] = torch.tensor([sd["slot"]])
    out["buf.prev_done"] = sd["prev_done"]
    out.update({f"buf.stored.{k}": v for k, v in sd["stored"].items()})
    out.update({f"buf.computed.{k}": v for k, v in sd.get("computed", {}).items()})
    if st.steps >= T:
        out.update({f"buf.flat.{k}": _host(v) for k, v in st.buf.flat().items()})
    out["vec.need_reset"] = _host(st.vec._need_reset)
    out["vec.episode_count"] = _host(st.vec.episode_count)
    out.update({f"net.{i}": _host(leaf) for i, leaf in enumerate(st.leaves)})
    out["loop.obs"] = _host(st.obs)
    return out


# ------------------------------------------------------------------------------------------------ checkpoints
def save(st: Stack, path, route: str = "adapter") -> None:
    """Every state dict, the network's leaves and the loop's variables through ``torch.save``.  ``route="adapter"``: the
    adapter's `state_dict`; ``route="parts"``: the dicts of the environment, the sampler and the normaliser one by one and
    nothing of the adapter's own -- all that the public calls offered before the adapter had a `state_dict`."""
    ck = {"head": st.head.state_dict(), "buf": st.buf.state_dict(), "ppo": st.ppo.state_dict(),
          "leaves": [_host(leaf) for leaf in st.leaves], "steps": st.steps, "pending": st.pending, "obs": _host(st.obs)}
    if route == "adapter":
        ck["vec"] = st.vec.state_dict()
    else:
        ck["env"] = st.env.state_dict()
        if st.sampler is not None:
            ck["episode_sampler"] = st.sampler.state_dict()
        if st.norm is not None:
            ck["normalizer"] = st.norm.state_dict()
    torch.save(ck, path)


def load(st: Stack, path) -> None:
    """Into ``st`` through the public calls only, read with ``weights_only=True``."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if "vec" in ck:
        st.vec.load_state_dict(ck["vec"])
    else:
        st.env.load_state_dict(ck["env"])
        if st.sampler is not None:
            st.sampler.load_state_dict(ck["episode_sampler"])
        if st.norm is not None:
            st.norm.load_state_dict(ck["normalizer"])
    st.head.load_state_dict(ck["head"])
    st.buf.load_state_dict(ck["buf"])
    st.ppo.load_state_dict(ck["ppo"])
    with torch.no_grad():
        for leaf, saved in zip(st.leaves, ck["leaves"]):
            leaf.copy_(saved)
            leaf.grad = None
    st.steps, st.pending, st.obs = int(ck["steps"]), bool(ck["pending"]), ck["obs"].to(st.device)


def fresh(variant: str, device: str, net_device: Optional[str] = None) -> Stack:
    """A new handle and new objects built with other seeds, dirtied by a reset and two control steps of their own."""
    st = Stack(variant, device, OTHER_SEEDS, net_device)
    run(st, 2, [], [])
    return st


# ------------------------------------------------------------------------------------------------ the uninterrupted run
_RUNS: dict = {}


def reference(variant: str, device: str, folder, net_device: Optional[str] = None) -> dict:
    """The uninterrupted run of ``K`` control steps, computed once per (variant, device, network device) and left unchanged:
    what every step and every PPO call handed out, `everything` at the end, and before every step the checkpoint files of
    both routes, the adapter's ``_need_reset`` and the sampler's draw counts."""
    key = (variant, device, net_device or device)
    if key not in _RUNS:
        st = Stack(variant, device, RUN_SEEDS, net_device)
        steps, calls, need, counts, paths = [], [], [], [], []
        for k in CUTS:
            run(st, k, steps, calls)
            paths.append({route: folder / f"{variant}-{device.replace(':', '')}-{net_device}-{route}-{k}.pt" for route in ("adapter", "parts")})
            for route, path in paths[-1].items():
                save(st, path, route)
            need.append(_host(st.vec._need_reset))
            counts.append(None if st.sampler is None else _host(st.sampler.draw_counts()))
        run(st, K, steps, calls)
        _RUNS[key] = dict(steps=steps, calls=calls, need=need, counts=counts, paths=paths, end=everything(st),
                          final_counts=None if st.sampler is None else _host(st.sampler.draw_counts()))
        st.close()
    return _RUNS[key]


def resume(variant: str, device: str, path, upto: int = K, net_device: Optional[str] = None):
    """A fresh stack loaded from ``path`` and continued to control step ``upto``: (stack, steps, calls) after the cut."""
    st = fresh(variant, device, net_device)
    load(st, path)
    steps, calls = [], []
    run(st, upto, steps, calls)
    return st, steps, calls


def check_resume(ref: dict, variant: str, device: str, k: int, net_device: Optional[str] = None) -> None:
    """The property: everything after cut ``k`` equals the uninterrupted run's on every byte."""
    st, steps, calls = resume(variant, device, ref["paths"][k]["adapter"], net_device=net_device)
    try:
        assert len(steps) == K - k
        for i, (got, want) in enumerate(zip(steps, ref["steps"][k:])):
            assert_equal(got, want, f"{variant}, cut {k}: what control step {k + i + 1} handed out")
        want_calls = [c for c in ref["calls"] if c["step"] >= k]
        assert [(c["step"], c["part"]) for c in calls] == [(c["step"], c["part"]) for c in want_calls]
        for got, want in zip(calls, want_calls):
            where = f"{variant}, cut {k}: PPO call {want['part']} after control step {want['step']}"
            assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, where)
        assert_equal(everything(st), ref["end"], f"{variant}, cut {k}: everything after control step {K}")
    finally:
        st.close()


def control_differences(ref: dict, variant: str, device: str) -> Dict[int, str]:
    """cut -> the first block that differs when the resume leaves the adapter's own two tensors out (``route="parts"``) and
    goes on for one control step: what that step handed out, then what the stack holds against the uninterrupted run's
    ``_need_reset`` after it."""
    out = {}
    for k in CUTS:
        st, steps, _ = resume(variant, device, ref["paths"][k]["parts"], upto=k + 1)
        try:
            bad = first_difference(steps[0], ref["steps"][k])
            if bad is not None:
                out[k] = f"what control step {k + 1} handed out: {bad}"
        finally:
            st.close()
    return out


def assert_honest(ref: dict, variant: str) -> None:
    """The conditions without which the property would hold for a tame reason, on the uninterrupted run."""
    need, steps, n = ref["need"], ref["steps"], ref["need"][0].shape[0]
    partial = [k for k in CUTS if 0 < int(need[k].sum()) < n]
    assert 2 * len(partial) >= len(CUTS), ("_need_reset is neither empty nor full at too few cuts", partial)
    term = torch.stack([s["terminated"] for s in steps])
    trunc = torch.stack([s["truncated"] for s in steps])
    done = term | trunc
    assert bool(term.any()) and bool(trunc.any()), "an environment terminates and an environment is truncated"
    assert any(0 < int(row.sum()) < n for row in done), "an environment ends in a step in which others do not"
    if variant == "host-reset":
        for counts in (ref["final_counts"], *[c for c in ref["counts"][1:]]):
            assert len(set(counts.tolist())) >= 3, counts
    if variant == "frozen":
        # cut 1: nobody is truncated yet, so every environment of `_need_reset` is terminated and its lane frozen
        assert not bool(trunc[0].any()) and 0 < int(need[1].sum()) < n, "frozen and live environments at a cut"
    second = [c for c in ref["calls"] if c["step"] == 2 * T]
    assert len(second) == 2 and len(ref["calls"]) == 4
    kl = STAT_NAMES.index("approx_kl")
    assert any(float(c["stats"][kl]) != 0.0 for c in second), "the ratios of the second rollout's PPO calls are not all 1"
    assert all(float(c["stats"][0]) > 0 and float(c["stats"][1]) == 0 and bool(c["stats"].isfinite().all()) for c in ref["calls"])


# ------------------------------------------------------------------------------------------------ the environment alone
ALONE = {"all-s13": lambda dev: snap.make(dev, 100, "all", "s13"), "all-s128": lambda dev: snap.make(dev, 100, "all", "s128"),
         "pulse-s13": lambda dev: snap.make(dev, 100, "pulse", "s13"), "pulse-s128": lambda dev: snap.make(dev, 100, "pulse", "s128"),
         "dynamic": lambda dev: episode_env(dev, 70)}


def check_mid_interval(which: str, device: str, path, kernel: int = 0, lanes: int = 0) -> WireEDMEnv:
    """1300 us (a control interval and 300 us: the accumulators in mid-interval), a checkpoint, 1200 us; against a fresh
    environment -- another seed, 100 us of its own -- loaded from the file and run the same 1200 us.  Returns the resumed
    environment (open) for the caller's own look at which kernel ran."""
    a, b = ALONE[which](device), ALONE[which](device)
    a.set_kernel(kernel, lanes)
    b.set_kernel(kernel, lanes)
    act = snap.scenario(a)
    a.step_many(act, 1300)
    a.save_checkpoint(path)
    a.step_many(act, 1200)
    b.step_many(snap.scenario(b, seed=78), 100)
    b.load_checkpoint(path)
    b.step_many(b.make_action(0.0, 80.0, 9, 3.0, 30.0), 1200)
    a.check_errors()
    b.check_errors()
    got, want = env_everything(b), env_everything(a)
    a.close()
    assert_equal(got, want, f"{which}, kernel {kernel} x {lanes} lanes: 1200 us after the checkpoint")
    done = b.state.done.cpu()
    assert int(b.state.spark_count.sum()) > 0 and 0 < int(done.sum()) < done.numel(), "the batch sparks; some environments are frozen"
    return b


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases(device: str):
    """[(name, word the message must hold, source adapter, target adapter)]: a dict of the source must be refused by the
    target.  Small environments: the refusals are host code."""
    plain = lambda n=6, **kw: snap.make(device, n, "plain", "s13", **kw)   # noqa: E731
    V = WireEDMVectorEnv
    base = dict(max_episode_steps=3000, wire_profile_bins=2)
    sampler = lambda: EpisodeSampler(7, params=RANGES, materials=True, height=HEIGHT, diameters=True)   # noqa: E731
    return [
        ("batch size", "num_envs", V(plain(), **base), V(plain(7), **base)),
        ("autoreset mode", "autoreset", V(plain(), **base), V(plain(), autoreset=False, **base)),
        ("max_episode_steps", "max_episode_steps", V(plain(), **base), V(plain(), max_episode_steps=2000, wire_profile_bins=2)),
        ("no max_episode_steps", "max_episode_steps", V(plain(), **base), V(plain(), wire_profile_bins=2)),
        ("profile bins", "wire_profile_bins", V(plain(), **base), V(plain(), max_episode_steps=3000, wire_profile_bins=3)),
        ("no profile bins", "wire_profile_bins", V(plain(), **base), V(plain(), max_episode_steps=3000)),
        ("observation columns", "obs_names", V(plain(), **base), V(snap.make(device, 6, "pulse", "s13"), **base)),
        ("reward", "reward", V(plain(), **base), V(plain(), reward="progress", **base)),
        ("sampler on the source only", "samplers", V(episode_env(device, 6), episode_sampler=sampler()), V(episode_env(device, 6))),
        ("sampler on the target only", "samplers", V(episode_env(device, 6)), V(episode_env(device, 6), episode_sampler=sampler())),
        ("normaliser on the source only", "normalizer", V(plain(), normalizer=Normalizer(), **base), V(plain(), **base)),
        ("normaliser on the target only", "normalizer", V(plain(), **base), V(plain(), normalizer=Normalizer(), **base)),
        # the nested dicts' own refusals, reached through the adapter
        ("the environment's physics", "physics", V(plain(), **base),
         V(plain(config=EnvironmentConfig(target_cutting_distance=4000.0)), **base)),
        ("the sampler's spec", "other names or from other ranges", V(episode_env(device, 6), episode_sampler=sampler()),
         V(episode_env(device, 6), episode_sampler=EpisodeSampler(7, params=RANGES, materials=True))),
    ]


def vec_everything(vec) -> Dict[str, torch.Tensor]:
    out = {f"env.{k}": v for k, v in env_everything(vec.env).items()}
    if vec._episode_sampler is not None:
        out.update({f"sampler.{k}": v for k, v in sampler_blocks(vec.env, vec._episode_sampler).items()})
    if vec.normalizer is not None:
        out["norm.stats"] = _host(vec.normalizer._stats)
        out.update({f"norm.rows.{k}": _host(v) for k, v in vec.normalizer.rows.items()})
    out["vec.need_reset"] = _host(vec._need_reset)
    out["vec.episode_count"] = _host(vec.episode_count)
    return out


def check_refusals(device: str) -> None:
    """Every mismatch raises ``ValueError`` with the word that names it, and no byte of the target changes."""
    for name, word, src, dst in refusal_cases(device):
        for vec, seed in ((src, 3), (dst, 4)):
            vec.reset(seed=seed)
            snap.scenario(vec.env, seed=seed)
            for _ in range(2):
                vec.step(vec.env.make_action(0.0, 80.0, 9, 3.0, 30.0))
        sd = src.state_dict()
        before = vec_everything(dst)
        try:
            dst.load_state_dict(sd)
        except ValueError as e:
            assert word in str(e), (name, str(e))
        else:
            raise AssertionError(f"{name}: the dict was accepted")
        assert_equal(vec_everything(dst), before, f"refused ({name}): the target changed")
        dst.load_state_dict(dst.state_dict())   # the target is whole: its own dict is accepted
        assert_equal(vec_everything(dst), before, f"{name}: the target's own dict")
        src.close()
        dst.close()
