"""Rollout storage and GAE on the MI355X (sparc_amd/csrc/wedm_gae.h, sparc_amd/rollout.py): `wedm_gae`
against `torch_gae` on every byte of everything it writes -- advantages, returns, valid mask, standardised advantages, tile
partials, moments and the done row -- at the wave, tile and unroll edges, with its blocks in guard bands; its two phases
apart and shards in turn against the whole batch; environments of mixed magnitude down to float32 subnormals, flag bytes
other than 0 and 1, a long rollout and the fold of a large workspace; and `RolloutBuffer` through `WireEDMVectorEnv`, without a host
synchronisation or an allocation per rollout."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from sparc_amd import RolloutBuffer, WireEDMVectorEnv, _abi
from sparc_amd.rollout import APPLY, NORMALIZE, SCAN, SCAN_UNROLL, SKIP_AFTER_DONE, device_gae, torch_gae
from tests._gae_common import FLAG_BYTES, GAE_KINDS, PAIRS, draw_mixed, is_subnormal, kinds_of
from tests._normalize_common import same_bits
from tests._snapshot_common import make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, BAND = 0xA5, 4096
U = SCAN_UNROLL
OUTPUTS = (("advantage", np.float32), ("returns", np.float32), ("valid", np.uint8), ("advantage_norm", np.float32))


class Banded:
    """A device block between two guard bands of 0xA5 bytes, holding a host array's bytes."""

    def __init__(self, host: np.ndarray):
        host = np.ascontiguousarray(host)
        self.nbytes = host.nbytes
        self.raw = torch.full((2 * BAND + -(-self.nbytes // 16) * 16,), FILL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[BAND: BAND + self.nbytes].view(torch.from_numpy(host).dtype).view(host.shape)
        self.t.copy_(torch.from_numpy(host))

    def bands_intact(self) -> bool:
        return bool((self.raw[:BAND] == FILL).all() and (self.raw[BAND + self.nbytes:] == FILL).all())


def poisoned(shape, dtype) -> np.ndarray:
    """An output block before the call: every byte 0xA5."""
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = FILL
    return a


class Problem:
    """One rollout of synthetic blocks on the device and the host: inputs ``[T, N + 5]`` with NaN (0xA5 in the flag blocks)
    in the padding columns, outputs ``[T, N + 3]`` of 0xA5 bytes, dones with probability 0.1 each.  `call` runs `wedm_gae`;
    `expect` builds, from `torch_gae` on the same data, every output block as the call has to leave it, padding included."""

    def __init__(self, N, T, seed, prev="given", n_tiles_total=None, p=0.1, gamma=0.99, lam=0.95, eps=1e-8, kinds=None):
        """``kinds``: None (unit normals and flag bytes 0 / 1), or the environments' kinds for `draw_mixed`."""
        self.N, self.T, self.prev_mode = N, T, prev
        rng = np.random.default_rng(seed)
        self.si, self.so = N + 5, N + 3
        self.kw = dict(gamma=gamma, lam=lam, eps=eps)
        self.tiles = -(-N // 256)
        self.n_tiles_total = self.tiles if n_tiles_total is None else n_tiles_total
        h = self.host = {}
        for name in ("reward", "value"):
            h[name] = np.full((T, self.si), np.nan, dtype=np.float32)
            h[name][:, :N] = rng.normal(size=(T, N))
        for name in ("terminated", "truncated"):
            h[name] = np.full((T, self.si), FILL, dtype=np.uint8)
            h[name][:, :N] = rng.random((T, N)) < p
        h["last_value"] = rng.normal(size=N).astype(np.float32)
        h["prev_done"] = (rng.random(N) < 0.2).astype(np.uint8)
        if kinds is not None:
            x = draw_mixed(rng, T, N, p, kinds)
            for name in ("reward", "value", "terminated", "truncated"):
                h[name][:, :N] = x[name]
            h["last_value"] = x["last_value"]
        self.inputs = {name: Banded(a) for name, a in h.items()}
        self.outputs = {name: Banded(poisoned((T, self.so), dt)) for name, dt in OUTPUTS}
        self.outputs["prev_done_out"] = Banded(poisoned((N,), np.uint8))
        self.outputs["partials"] = Banded(poisoned((self.n_tiles_total, 3), np.float64))
        self.outputs["moments"] = Banded(poisoned((3,), np.float64))

    def prev_host(self):
        return None if self.prev_mode == "null" else self.host["prev_done"]

    def desc(self, flags, lo=0, count=None, tile_offset=0):
        """The descriptor of environments [lo, lo + count): a shard is the same blocks entered ``lo`` elements further on."""
        count = self.N - lo if count is None else count
        at = lambda b: b.t.data_ptr() + lo * b.t.element_size()
        i, o = self.inputs, self.outputs
        prev_in = None if self.prev_mode == "null" else at(i["prev_done"])
        prev_out = prev_in if self.prev_mode == "aliased" else at(o["prev_done_out"])
        return _abi.GaeDesc(
            reward=at(i["reward"]), value=at(i["value"]), last_value=at(i["last_value"]), terminated=at(i["terminated"]),
            truncated=at(i["truncated"]), prev_done_in=prev_in, advantage=at(o["advantage"]), returns=at(o["returns"]),
            advantage_norm=at(o["advantage_norm"]), valid=at(o["valid"]), prev_done_out=prev_out,
            partials=o["partials"].t.data_ptr(), moments=o["moments"].t.data_ptr(), in_stride=self.si, out_stride=self.so,
            T=self.T, num_envs=count, tile_offset=tile_offset, n_tiles_total=self.n_tiles_total, flags=flags, **self.kw)

    def call(self, flags, **kw):
        device_gae(self.desc(flags, **kw), DEV)

    def expect(self, flags, partials=None, tile_offset=0):
        """Every output block as a whole-batch call with ``flags`` (both phases) has to leave it."""
        h = self.host
        out = torch_gae(h["reward"], h["value"], h["last_value"], h["terminated"], h["truncated"], num_envs=self.N,
                        prev_done=self.prev_host(), partials=poisoned((self.n_tiles_total, 3), np.float64) if partials is None else partials,
                        tile_offset=tile_offset, n_tiles_total=self.n_tiles_total, gamma=self.kw["gamma"], gae_lambda=self.kw["lam"],
                        eps=self.kw["eps"], flags=flags)
        self.out = out
        want = {}
        for name, dt in OUTPUTS:
            want[name] = poisoned((self.T, self.so), dt)
            if name in out:
                want[name][:, : self.N] = out[name].numpy()
        want["prev_done_out"] = poisoned((self.N,), np.uint8) if self.prev_mode == "aliased" else out["prev_done_out"].numpy()
        want["prev_done"] = out["prev_done_out"].numpy() if self.prev_mode == "aliased" else h["prev_done"]
        normalize = bool(flags & NORMALIZE)
        want["partials"] = out["partials"].numpy() if normalize else poisoned((self.n_tiles_total, 3), np.float64)
        want["moments"] = out["moments"].numpy() if normalize else poisoned((3,), np.float64)
        return want

    def differences(self, want):
        """Names of the blocks -- outputs, and inputs, which nothing may change -- whose bytes differ from ``want`` / the host's."""
        torch.cuda.synchronize()
        got = {**{k: b.t for k, b in self.outputs.items()}, **{k: b.t for k, b in self.inputs.items()}}
        ref = {**self.host, **want}
        bad = [name for name, t in got.items() if not same_bits(t, ref[name])]
        return bad + [f"band of {name}" for name, b in {**self.inputs, **self.outputs}.items() if not b.bands_intact()]


# ------------------------------------------------------------------------------------------------ the call on synthetic blocks
STEPS = (1, 2, U - 1, U, U + 1, 2 * U + 1, 3 * U + 2)
FLAGS = (SKIP_AFTER_DONE | NORMALIZE, 0, SKIP_AFTER_DONE, NORMALIZE)
PREV = ("null", "given", "aliased")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 513])
def test_the_call_equals_the_definition_on_every_byte(N):
    """The wave (64) and tile (256) edges by every length of the time loop around the unroll depth U (tail only, one chunk,
    a chunk and a tail, two and three chunks and a tail: the kernel loads a chunk while the one before it computes), every
    combination of the two option flags, and prev_done_in NULL, given and the same pointer as prev_done_out: 7 x 4 x 3 calls.  The blocks lie in guard bands, outputs start as 0xA5 bytes, the
    padding columns [num_envs, stride) hold NaN (inputs) and must come out as they were."""
    seen = dict(cut_chain=0, skipped_step=0, bootstrap_at_last_step=0, terminated_at_last_step=0)
    for T in STEPS:
        for flags in FLAGS:
            for prev in PREV:
                p = Problem(N, T, seed=1000 * N + 100 * T + 10 * flags + PREV.index(prev), prev=prev)
                want = p.expect(flags)
                p.call(flags)
                assert p.differences(want) == [], (N, T, flags, prev)
                te, tr = (p.host[k][:, :N].astype(bool) for k in ("terminated", "truncated"))
                seen["cut_chain"] += int((te | tr)[:-1].sum())
                seen["skipped_step"] += int((p.out["valid"] == 0).sum())
                seen["bootstrap_at_last_step"] += int((tr & ~te)[-1].sum())
                seen["terminated_at_last_step"] += int(te[-1].sum())
    assert all(count > 0 for count in seen.values()), seen


def test_scan_and_apply_as_separate_calls_equal_the_combined_call():
    both = SKIP_AFTER_DONE | NORMALIZE
    whole, parts = Problem(513, U + 3, seed=50), Problem(513, U + 3, seed=50)
    want = whole.expect(both)
    whole.call(both)
    assert whole.differences(want) == []
    parts.call(both | SCAN)
    torch.cuda.synchronize()
    assert bool((parts.outputs["moments"].raw == FILL).all()) and bool((parts.outputs["advantage_norm"].raw == FILL).all())
    assert same_bits(parts.outputs["partials"].t, whole.outputs["partials"].t)
    parts.call(both | APPLY)
    assert parts.differences(want) == []
    assert all(same_bits(parts.outputs[k].raw, whole.outputs[k].raw) for k in whole.outputs)


@pytest.mark.parametrize("n_tiles_total", [4, 5])
def test_shards_in_turn_equal_the_whole_batch(n_tiles_total):
    """769 environments as one call, and as shards of 512 + 257 that each SCAN into their tiles (0-1 and 2-3) of one shared
    workspace and then each APPLY: what an all-gather of the partials between the two phases gives several devices.  769
    environments fill four tiles; the workspace of five has a spare one, left EMPTY by zeroing."""
    both = SKIP_AFTER_DONE | NORMALIZE
    whole, parts = (Problem(769, 6, seed=51, n_tiles_total=n_tiles_total) for _ in range(2))
    zeroed = np.zeros((n_tiles_total, 3))
    for p in (whole, parts):
        p.outputs["partials"].t.zero_()
    want = whole.expect(both, partials=zeroed)
    whole.call(both)
    assert whole.differences(want) == []
    for phase in (SCAN, APPLY):
        parts.call(both | phase, lo=0, count=512, tile_offset=0)
        parts.call(both | phase, lo=512, count=257, tile_offset=2)
    assert parts.differences(want) == []
    assert all(same_bits(parts.outputs[k].raw, whole.outputs[k].raw) for k in whole.outputs)
    assert float(whole.outputs["moments"].t[0]) == float(want["valid"][:, :769].sum()) > 0


def test_a_batch_with_every_step_skipped():
    p = Problem(300, 5, seed=52, p=1.0)
    p.host["prev_done"][:] = 1
    p.inputs["prev_done"].t.fill_(1)
    flags = SKIP_AFTER_DONE | NORMALIZE
    want = p.expect(flags)
    p.call(flags)
    assert p.differences(want) == []
    o = p.outputs
    assert o["moments"].t.tolist() == [0.0, 0.0, 0.0] and not bool(o["partials"].t.any())
    assert not bool(o["advantage_norm"].t[:, :300].any()) and not bool(o["advantage"].t[:, :300].any())
    assert not bool(o["valid"].t[:, :300].any())
    assert not any(bool(torch.isnan(o[k].t[:, :300]).any()) for k in ("advantage", "returns", "advantage_norm"))


def test_run_twice_gives_the_same_bits():
    got = []
    for _ in range(2):
        p = Problem(1000, 2 * U + 3, seed=53)
        p.call(SKIP_AFTER_DONE | NORMALIZE)
        torch.cuda.synchronize()
        got.append({name: b.raw.clone() for name, b in p.outputs.items()})
    assert all(same_bits(got[0][name], got[1][name]) for name in got[0])


# ------------------------------------------------------------------------------------------------ magnitudes, lengths, folds
def finite(p):
    """The condition under which `wedm_gae` is compared on every byte: the definition's outputs (``p.out``, after `expect`)
    hold no NaN and no infinity -- `wedm_gae` does not canonicalise a NaN, and the header leaves a NaN's numbers unspecified."""
    return all(bool(torch.isfinite(t.to(torch.float64)).all()) for t in p.out.values())


@pytest.mark.parametrize("N", [1, 65, 257, 513])
def test_mixed_kinds_equal_the_definition_on_every_byte(N):
    """Environments of `GAE_KINDS` -- normal, offset 1e6 + U(0, 8), constant 293.15, tiny 1e-30, huge 1e30, subnormal 1e-41,
    signed zeros, independently in ``reward``, ``value`` and ``last_value`` -- with ``terminated`` / ``truncated`` bytes
    from {0, 1, 2, 0x80, 0xFF} (non-zero means set; ``prev_done_out`` is still exactly 0 or 1), for T in {1, U + 1, 3U + 2}
    by (gamma, lam) in {(0.99, 0.95), (1, 1), (0, 0.5), (0.97, 0)} by both option flags and none.  Float32 subnormals are
    read and stored: the definition keeps them, and so must the kernels."""
    seen_kinds, seen_bytes, subnormal = set(), set(), dict(advantage=0, returns=0, advantage_norm=0)
    for T in (1, U + 1, 3 * U + 2):
        for gamma, lam in PAIRS:
            for flags in (SKIP_AFTER_DONE | NORMALIZE, 0):
                p = Problem(N, T, seed=7000 * N + 100 * T + 10 * PAIRS.index((gamma, lam)) + flags, gamma=gamma, lam=lam, kinds=GAE_KINDS)
                want = p.expect(flags)
                assert finite(p), (N, T, gamma, lam, flags)
                p.call(flags)
                assert p.differences(want) == [], (N, T, gamma, lam, flags)
                assert set(want["prev_done_out"].tolist()) <= {0, 1} and set(want["valid"][:, :N].reshape(-1).tolist()) <= {0, 1}
                for name in ("terminated", "truncated"):
                    seen_bytes |= set(p.host[name][:, :N].reshape(-1).tolist())
                for kinds in kinds_of(N):
                    seen_kinds |= set(kinds.tolist())
                for name in subnormal:
                    if name in p.out:
                        subnormal[name] += int(is_subnormal(p.out[name].numpy()).sum())
    if N > 1:   # (one environment is of the first kind, and may never set a flag)
        assert seen_kinds == set(range(len(GAE_KINDS))) and seen_bytes == set(FLAG_BYTES)
        assert subnormal["advantage"] > 0 and subnormal["returns"] > 0, subnormal


def test_a_long_rollout_equals_the_definition_on_every_byte():
    """T = 40 U + 3 at N = 65 with normal and offset environments: the pipelined chunk loop runs 39 iterations (the tests
    above: at most two) before its last chunk and the three steps that fill none."""
    flags = SKIP_AFTER_DONE | NORMALIZE
    p = Problem(65, 40 * U + 3, seed=60, p=0.02, kinds=("normal", "offset"))
    want = p.expect(flags)
    assert finite(p)
    p.call(flags)
    assert p.differences(want) == []
    assert 0 < int(want["valid"][:, :65].sum()) < 65 * (40 * U + 3) and float(want["moments"][0]) == float(want["valid"][:, :65].sum())


@pytest.mark.parametrize("n_tiles_total", [256, 257, 1025, 4096])
def test_the_fold_of_a_large_workspace(n_tiles_total):
    """As tests/test_normalize.py's: the fold gives a lane 1, 2, 8 or 16 tiles of the one-column workspace (``per`` of
    `wedm_norm_fold_tiles`), on other shards' nodes, a third of them EMPTY, around this batch's two tiles; SCAN then APPLY
    at ``tile_offset = n_tiles_total - 2`` against `torch_gae` given the same workspace."""
    both = SKIP_AFTER_DONE | NORMALIZE
    p = Problem(300, U + 1, seed=61, n_tiles_total=n_tiles_total)
    rng = np.random.default_rng(n_tiles_total)
    nodes = np.stack([rng.integers(1, 257, n_tiles_total).astype(np.float64), rng.normal(size=n_tiles_total),
                      rng.uniform(0.0, 50.0, n_tiles_total)], axis=1)
    nodes[rng.random(n_tiles_total) < 0.33] = 0.0
    p.outputs["partials"].t.copy_(torch.from_numpy(nodes))
    offset = n_tiles_total - 2
    want = p.expect(both, partials=nodes, tile_offset=offset)
    assert finite(p) and want["moments"][0] > nodes[:offset, 0].sum() > 0
    assert same_bits(want["partials"][:offset], nodes[:offset]) and not same_bits(want["partials"][offset:], nodes[offset:])
    p.call(both | SCAN, tile_offset=offset)
    p.call(both | APPLY, tile_offset=offset)
    assert p.differences(want) == []


@pytest.mark.parametrize("prev_done", [0, 1])
def test_one_environment_and_one_step(prev_done):
    """N = 1, T = 1 with the default eps: one valid step gives S exactly 0 and the denominator sqrt(eps), and the one
    standardised advantage is (A - A) / sqrt(eps) = 0; after a done nothing is valid and the moments are EMPTY."""
    for flags in (SKIP_AFTER_DONE | NORMALIZE, NORMALIZE, SKIP_AFTER_DONE, 0):
        p = Problem(1, 1, seed=62 + flags)
        p.host["prev_done"][:] = prev_done
        p.inputs["prev_done"].t.fill_(prev_done)
        want = p.expect(flags)
        p.call(flags)
        assert p.differences(want) == [], flags
        if flags & NORMALIZE:
            skipped = bool(prev_done and flags & SKIP_AFTER_DONE)
            a = float(want["advantage"][0, 0])
            assert want["moments"].tolist() == ([0.0, 0.0, 0.0] if skipped else [1.0, a, 0.0]) and float(want["advantage_norm"][0, 0]) == 0.0
            assert skipped or a != 0.0


# ------------------------------------------------------------------------------------------------ through the adapter
def test_rollout_buffer_through_the_vector_env():
    """96 environments x 128 segments with in-kernel autoreset and progress reward, episodes of three control intervals,
    rollouts of six steps with values from a seeded generator: `finish` equals `torch_gae` of the host copies, ``valid`` is 0
    exactly at the steps after a done, and a second rollout neither synchronises with the host nor allocates."""
    n, T = 96, 6
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s128"), max_episode_steps=3000)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    assert buf._native is not None
    gen = torch.Generator(device=DEV).manual_seed(3)
    values = torch.randn(2 * T + 2, n, generator=gen, device=DEV)
    obs, _ = vec.reset(seed=21)
    vec.env.state.workpiece_position = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=DEV)
    vec.env.state.wire_position = 10.0
    action = vec.env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    steps = []

    def rollout(k, keep):
        nonlocal obs
        for t in range(T):
            value = values[k * T + t]
            nxt, reward, term, trunc, _ = vec.step(action)
            buf.add(obs, action, value, reward, term, trunc, log_prob=value)
            if keep:
                steps.append((obs, value, reward, term, trunc))
            obs = nxt
        return buf.finish(values[2 * T + k])

    first = {k: v.clone() for k, v in rollout(0, True).items()}
    stored = {k: v.clone() for k, v in buf.stored.items()}
    torch.cuda.synchronize()
    gc.collect()   # `memory_allocated` counts the whole process: earlier tests' environments are collected first
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        second = rollout(1, False)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    prev = np.zeros(n, dtype=np.uint8)
    for k, (got, blocks) in enumerate(((first, stored), (second, buf.stored))):
        want = torch_gae(blocks["reward"], blocks["value"], values[2 * T + k], blocks["terminated"], blocks["truncated"], prev_done=prev)
        for name in ("advantage", "advantage_norm", "returns"):
            assert same_bits(got[name], want[name]), (k, name)
        assert torch.equal(got["valid"].cpu(), want["valid"].bool())
        done = (blocks["terminated"] | blocks["truncated"]).cpu()
        assert torch.equal(got["valid"].cpu(), ~torch.cat([torch.from_numpy(prev).bool()[None], done[:-1]]))
        prev = want["prev_done_out"].numpy()
        assert done.any() and not got["valid"].all() and float(blocks["reward"].abs().sum()) > 0
    assert same_bits(buf.prev_done, prev) and same_bits(buf.moments, want["moments"])
    for j, name in enumerate(("obs", "value", "reward", "terminated", "truncated")):   # what reset / step returned
        assert same_bits(stored[name], torch.stack([s[j] for s in steps])), name
    assert same_bits(stored["action.servo"], torch.full((T, n), 0.1, dtype=torch.float64))
    assert after == before, (before, after)
