"""`wedm_episode_log` on the MI355X: the call against `episode_log_definition` on every byte of an arena
that holds all its blocks between guard bands -- the ring, the accumulators, ``tile_counts``, ``head``, padding columns, the
inputs -- at the wave and block edges, with bases on and off 16 bytes, at the plane and row limits, the phases apart and two
shards in turn; a small shard in workspaces of 64 to 4096 tiles, whole batches past one pass over ``tile_counts`` and a head
past 32 bits; `EpisodeLog` through `WireEDMVectorEnv` without a host synchronisation or an allocation, against its twin
on the CPU oracle backend; and the call on a side stream behind a gate."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from sparc_amd import EpisodeLog, Normalizer, WireEDMVectorEnv
from sparc_amd.episode_log import COMMIT, COUNT, SCATTER, device_episode_log
from tests import _snapshot_common as snap
from tests._episode_log_common import (CAPS, DRAWS, SHARD_N, SPEC_MAX, SPEC_SHARD, WHERE, WORKSPACES, Problem, differences, finishing,
                                        flags_from, full_stack, shard_case)
from tests._stream_gate import Gate, check_control, gated, seconds_on

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class OnDevice:
    """A problem's arena on the device, and its twin on the host that the definition moves on."""

    def __init__(self, p: Problem):
        self.p, self.want = p, p.buf.copy()
        self.dev = torch.from_numpy(p.buf.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def flags(self, term, trunc, mask) -> None:
        got = self.dev.cpu().numpy()
        for buf in (got, self.want):
            self.p.set_flags(buf, term, trunc, mask)
        self.dev.copy_(torch.from_numpy(got))

    def call(self, **kw) -> None:
        device_episode_log(self.p.desc(self.dev.data_ptr(), **kw), DEV)

    def check(self, where) -> None:
        assert differences(self.p, self.dev.cpu().numpy(), self.want) == [], where


@pytest.mark.parametrize("how", ["none", "first", "last", "few", "all"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_call_against_the_definition_on_every_byte(N, how):
    """Capacity 1, 7, 256 and num_envs + 5; source strides of num_envs and num_envs + 3; bases on and off 16 bytes; with and
    without a mask and ``truncated``.  Per case: the call, the same call again, and a call with a few finishing, so that the
    ring wraps across calls."""
    rng = np.random.default_rng(2000 * N + len(how))
    for case, cap in enumerate((1, 7, 256, N + 5)):
        masked, with_trunc = (case + N) % 2 == 0, (case + len(how)) % 3 != 0
        p = Problem(rng, N, cap, pad=3 * (case % 2), off16=case in (1, 2), head0=int(rng.integers(0, 50)), truncated=with_trunc,
                    masked=masked)
        d = OnDevice(p)
        fin = finishing(rng, N, how)
        for call, fin in enumerate((fin, fin, finishing(rng, N, "few"))):
            if call != 1:   # (call 1 is call 0 again, flags and all)
                mask = (rng.random(N) < 0.8).astype(np.uint8) if masked else None
                term, trunc = flags_from(rng, fin, mask)
                if not with_trunc:
                    term, trunc = term | trunc, None
                d.flags(term, trunc, mask)
            d.call(stamp=20 + call, env_id_offset=4000)
            p.define(d.want, stamp=20 + call, env_id_offset=4000)
            d.check((N, how, cap, call))


# ------------------------------------------------------------------------------------------------ large workspaces
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ntt", WORKSPACES)
def test_a_small_shard_in_a_large_workspace(ntt, where, draw, cap):
    """300 environments at the start, near the middle and at the end of a workspace of 64 to 4096 tiles whose other tiles
    hold counts that `shard_case` drew: SCATTER's and COMMIT's sums over ``tile_counts`` run one pass, two and sixteen (or
    64), the ranks start at up to 900 000 and ``head`` moves by as much.  One call, and COUNT, SCATTER, COMMIT apart; two
    calls each, on a ring entered two slots before its end.  tests/test_episode_log_host.py asserts the input conditions
    over the parametrisation: records all stored, none stored, a strict part."""
    offset, others, calls, capacity, _, totals = shard_case(ntt, where, draw, cap)
    p = Problem(np.random.default_rng(ntt + capacity), SHARD_N, capacity, tile_offset=offset, n_tiles_total=ntt, head0=capacity - 2,
                masked=True, pad=3, off16=where == "middle")
    p.view(p.buf, "tile_counts")[:] = others
    for apart in (False, True):
        d = OnDevice(p)
        for call, (term, trunc, mask) in enumerate(calls):
            d.flags(term, trunc, mask)
            for phase in (COUNT, SCATTER, COMMIT) if apart else (0,):
                d.call(stamp=call, env_id_offset=9000, flags=phase)
            p.define(d.want, stamp=call, env_id_offset=9000)
            d.check((ntt, where, draw, cap, apart, call))
        head = p.view(d.want, "head")
        assert head[0] == capacity - 2 + sum(totals) and head[1] == totals[1]


@pytest.mark.parametrize("N,cap", [(16_385, 300), (16_641, 300), (16_641, 16_646), (65_537, 300), (65_793, 300), (65_793, 65_798)])
def test_whole_batches_past_one_pass_over_the_tile_counts(N, cap):
    """65 and 66 tiles, 257 and 258: one and two more than COMMIT's 64 lanes and than SCATTER's 256 take in a pass, the last
    tile of one environment: "few", "all", "few" with a mask, on a ring that drops most records and on one that holds them
    all, entered two slots before its end."""
    rng = np.random.default_rng(N + cap)
    p = Problem(rng, N, cap, masked=True, pad=3, off16=cap == 300, head0=cap - 2)
    assert p.tiles in (65, 66, 257, 258) and p.ntt == p.tiles
    d = OnDevice(p)
    for call, how in enumerate(("few", "all", "few")):
        mask = (rng.random(N) < 0.8).astype(np.uint8)
        if how == "all":
            mask[-1] = 1   # the one environment of the last tile finishes: the tile past the first pass counts
        d.flags(*flags_from(rng, finishing(rng, N, how), mask), mask)
        d.call(stamp=call, env_id_offset=12)
        p.define(d.want, stamp=call, env_id_offset=12)
        d.check((N, cap, call))
        if how == "all":
            counts = p.view(d.want, "tile_counts")
            assert p.view(d.want, "head")[1] > 0.7 * N and (counts[: p.tiles - 1] > 150).all() and counts[-1] == 1


@pytest.mark.parametrize("cap", [7, 100, 256])
@pytest.mark.parametrize("head0", [2 ** 40 + 3, 2 ** 31 - 1])
def test_a_head_past_32_bits(head0, cap):
    """``head[0]`` where `EpisodeLog` leaves it after 2^31 and 2^40 episodes: the slot is ``(head[0] + k) mod capacity`` in 64 bits.
    At 257 environments and capacities 7 and 100 the slot of the sum's low 32 bits is another one (2^31 and 2^40 leave
    remainders there; a capacity of 256 divides both, so its slots alone could not tell)."""
    N = 257
    rng = np.random.default_rng(cap)
    assert cap == 256 or (head0 + 1) % cap != (np.int64(head0 + 1).astype(np.int32).item()) % cap
    p = Problem(rng, N, cap, masked=True, pad=3, head0=head0)
    d = OnDevice(p)
    for call, how in enumerate(("all", "few")):
        mask = (rng.random(N) < 0.8).astype(np.uint8)
        d.flags(*flags_from(rng, finishing(rng, N, how), mask), mask)
        d.call(stamp=call)
        p.define(d.want, stamp=call)
        d.check((head0, cap, call))
    assert p.view(d.want, "head")[0] > head0 + 100


@pytest.mark.parametrize("N,cap", [(257, 7), (1000, 1005), (1000, 300), (65_793, 1000)])
def test_the_maximum_plane_and_row_counts(N, cap):
    rng = np.random.default_rng(N + cap)
    p = Problem(rng, N, cap, spec=SPEC_MAX, pad=3, off16=True, masked=True, head0=cap - 2)
    d = OnDevice(p)
    for call, how in enumerate(("few", "all", "few")):
        mask = (rng.random(N) < 0.8).astype(np.uint8)
        d.flags(*flags_from(rng, finishing(rng, N, how), mask), mask)
        d.call(stamp=call)
        p.define(d.want, stamp=call)
        d.check((N, cap, call))


@pytest.mark.parametrize("N,cap", [(1, 1), (257, 7), (1000, 100)])
def test_the_phases_apart(N, cap):
    """Three calls of one phase each against the definition's one call; then each phase alone against the definition's."""
    rng = np.random.default_rng(N + cap + 1)
    p = Problem(rng, N, cap, masked=True, head0=3, pad=3)
    d = OnDevice(p)
    for call, how in enumerate(("all", "few")):
        mask = (rng.random(N) < 0.7).astype(np.uint8)
        d.flags(*flags_from(rng, finishing(rng, N, how), mask), mask)
        for phase in (COUNT, SCATTER, COMMIT):
            d.call(stamp=call, flags=phase)
        p.define(d.want, stamp=call)
        d.check((N, cap, call))
    for phase in (COMMIT, COUNT, SCATTER):
        d.call(stamp=7, flags=phase)
        p.define(d.want, stamp=7, flags=phase)
        d.check((N, cap, "alone", phase))


@pytest.mark.parametrize("N,first", [(768, 256), (1000, 512)])
def test_shards_in_turn_equal_the_whole_batch(N, first):
    """COUNT every shard into its tiles of one workspace, SCATTER every shard, COMMIT once: the bytes of the whole-batch
    definition."""
    rng = np.random.default_rng(N)
    parts = ((0, first), (first, N - first))
    for cap in (5, 2000):
        p = Problem(rng, N, cap, spec=SPEC_SHARD, masked=True, head0=11, pad=2)
        d = OnDevice(p)
        for call, how in enumerate(("few", "all", "few")):
            mask = (rng.random(N) < 0.8).astype(np.uint8)
            d.flags(*flags_from(rng, finishing(rng, N, how), mask), mask)
            for phase in (COUNT, SCATTER):
                for part in parts:
                    d.call(stamp=call, env_id_offset=70, flags=phase, part=part)
            d.call(stamp=call, env_id_offset=70, flags=COMMIT, part=parts[1])
            p.define(d.want, stamp=call, env_id_offset=70)
            d.check((N, cap, call))


# ------------------------------------------------------------------------------------------------ the stack
def in_kernel_stack(device: str, capacity: int):
    """64 environments of 13 segments that reset inside the step kernel, with a normaliser and the wire profile: a `step()`
    without any host synchronisation."""
    env = snap.make(device, 64, "autoreset", "s13")
    log = EpisodeLog(capacity=capacity)
    vec = WireEDMVectorEnv(env, max_episode_steps=3000, wire_profile_bins=2, normalizer=Normalizer(gamma=0.9, clip_obs=5.0),
                           episode_log=log)
    vec.reset(seed=33)
    return vec, log, snap.scenario(env, seed=77)


def same_records(got: dict, want: dict, where) -> None:
    assert list(got) == list(want), where
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, key)


def test_steps_with_a_log_neither_synchronise_nor_allocate_and_equal_the_oracle_twin():
    reads = {}
    for device in (DEV, "cpu"):
        vec, log, action = in_kernel_stack(device, 256)
        vec.step(action)
        allocated = []
        if device == DEV:
            assert log._native is not None
            torch.cuda.synchronize()
            gc.collect()
            gc.disable()
            torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(6):
                vec.step(action)
                allocated.append(torch.cuda.memory_allocated())
        finally:
            if device == DEV:
                torch.cuda.set_sync_debug_mode("default")
                gc.enable()
        if device == DEV:
            torch.cuda.synchronize()
            assert allocated[1:] == [allocated[1]] * 5, allocated
        vec.env.check_errors()
        reads[device] = log.read()
        vec.close()
    got, want = reads[DEV], reads["cpu"]
    same_records(got, want, "in-kernel stack")
    assert want["lost"] == 0 and want["terminated"].any() and want["truncated"].any() and len(want["env"]) > 64
    assert len(set(want["stamp"].tolist())) > 2 and want["steps"].max() == 3, "episodes end in several steps, after up to three"


def test_the_log_of_a_stack_with_every_optional_block_equals_the_oracle_twin():
    reads = {}
    for device in (DEV, "cpu"):
        vec, log, action = full_stack(device, 4096, n=70)
        for _ in range(5):
            vec.step(action)
        vec.env.check_errors()
        reads[device] = log.read()
        vec.close()
    want = reads["cpu"]
    same_records(reads[DEV], want, "stack with every optional block")
    assert want["lost"] == 0 and want["wire_broken"].any() and want["target_reached"].any() and want["truncated"].any()
    assert {"draw", "material", "height", "diameter_index", "return", "length", "sparks", "energy", "envp_max_speed"} <= set(want)


# ------------------------------------------------------------------------------------------------ on a side stream
def test_episode_log_behind_the_gate():
    """257 environments (a block of 256 and a block with one live lane) with a mask, on a ring of 7 that wraps; ``terminated``
    is the gated input.  The control is a twin problem reading the same ``terminated`` on the default stream."""
    N, cap = 257, 7
    rng = np.random.default_rng(40)
    p = Problem(rng, N, cap, masked=True, head0=5, pad=3)
    mask = (rng.random(N) < 0.8).astype(np.uint8)
    term_a, trunc = flags_from(rng, finishing(rng, N, "few"), mask)
    term_b, _ = flags_from(rng, finishing(rng, N, "all"), mask)
    trunc[:] = 0
    shared = torch.from_numpy(term_a.copy()).to(DEV)
    dev_b = torch.from_numpy(term_b.copy()).to(DEV)
    under, control, warm = OnDevice(p), OnDevice(p), OnDevice(p)
    for d in (under, control, warm):
        d.flags(term_a, trunc, mask)

    def call(d):
        desc = p.desc(d.dev.data_ptr(), stamp=3)
        desc.terminated = shared.data_ptr()
        device_episode_log(desc, DEV)

    call(warm)
    gate = Gate(seconds_on(torch.cuda.default_stream(), lambda: call(warm)))
    want_a, want_b = p.buf.copy(), p.buf.copy()
    p.set_flags(want_a, term_a, trunc, mask)
    p.set_flags(want_b, term_b, trunc, mask)
    p.define(want_a, stamp=3)
    p.define(want_b, stamp=3)
    outputs = [name for name in p.layout if name.startswith(("dst", "acc")) or name in ("env_out", "stamp_out", "head", "tile_counts")]
    assert all(p.view(want_a, name).tobytes() != p.view(want_b, name).tobytes() for name in ("head", "tile_counts", "env_out"))
    gated(gate, lambda: shared.copy_(dev_b), lambda: call(under), lambda: call(control))
    # the arenas' own `terminated` blocks hold A and are not read: the expected arenas differ from A's in the outputs only
    p.set_flags(want_b, term_a, trunc, mask)
    assert differences(p, under.dev.cpu().numpy(), want_b) == [], "wedm_episode_log behind the gate"
    got = control.dev.cpu().numpy()
    check_control(all(p.view(got, name).tobytes() == p.view(want_a, name).tobytes() for name in outputs),
                  any(p.view(got, name).tobytes() == p.view(want_b, name).tobytes() for name in ("head", "tile_counts", "env_out")),
                  gate, "wedm_episode_log")
