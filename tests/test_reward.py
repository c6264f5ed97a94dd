"""`wedm_reward` on the MI355X (sparc_amd/csrc/wedm_reward.h): the call against `reward_definition` on
every byte of an arena that holds all its blocks between guard bands -- the two outputs, padding columns, the inputs -- at the
wave and block edges, with bases on and off 16 bytes, with and without ``mask``, ``restart`` and ``terms_out``, with every
term on, each term alone beside NULL blocks and none; hostile rows; two shards in turn; the call on a side stream behind a
gate; `ShapedReward` through `WireEDMVectorEnv` without a host synchronisation or an allocation against its twin on the CPU
oracle backend; and a training run with the shaped reward on the GPU against the same run on the oracle backend."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from sparc_amd import _abi
from sparc_amd.reward import device_reward
from tests import _resume_common as rc
from tests._reward_common import ALL_ON, ALL_ZERO, Problem, alone, differences, in_kernel_stack, run_whole
from tests._stream_gate import Gate, check_control, gated, seconds_on

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = _abi.RW_COUNT


class OnDevice:
    """A problem's arena on the device, and its twin on the host that the definition moves on."""

    def __init__(self, p: Problem):
        self.p, self.want = p, p.buf.copy()
        self.dev = torch.from_numpy(p.buf.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def call(self, weights=ALL_ON, **kw) -> None:
        device_reward(self.p.desc(self.dev.data_ptr(), weights, **kw), DEV)
        self.p.define(self.want, weights, **kw)

    def check(self, where) -> None:
        assert differences(self.p, self.dev.cpu().numpy(), self.want) == [], where


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_call_against_the_definition_on_every_byte(N):
    """Strides of num_envs and num_envs + 3, for the state blocks and for ``terms_out``; bases on and off 16 bytes; every
    combination of ``mask``, ``restart`` and ``terms_out`` present or NULL.  Per case: every term on, every weight zero, a
    random subset with random weights, and each term alone with the blocks it does not read NULL."""
    rng = np.random.default_rng(3000 + N)
    for case in range(8):
        p = Problem(rng, N, pad=3 * (case % 2), terms_pad=3 * ((case // 2) % 2), off16=case in (1, 2, 5, 6), masked=bool(case & 1),
                    restart=bool(case & 2), terms=not case & 4 or case == 7)
        d = OnDevice(p)
        subset = tuple(rng.standard_normal(K) * (rng.random(K) < 0.6))
        for weights, nulls in ((ALL_ON, False), (ALL_ZERO, True), (subset, True), (ALL_ZERO, False)):
            d.call(weights, nulls=nulls)
            d.check((N, case, weights, nulls))
        if case in (0, 3, 5, 7):
            for k in range(K):
                d.call(alone(k), nulls=True)
                d.check((N, case, "alone", k))
    # every weight zero: +0.0 everywhere
    d.call(ALL_ZERO, nulls=True)
    assert not p.view(d.dev.cpu().numpy(), "reward_out").view(np.uint32).any() and not p.view(d.want, "terms_out")[:, :N].view(np.uint64).any()
    d.check((N, "zero"))


@pytest.mark.parametrize("masked", [False, True])
def test_hostile_rows_at_257_environments(masked):
    """NaNs of two payloads, infinities, subnormals, both zeros and the largest numbers in the position row, ``pos_before`` and
    the signal rows; INT32_MIN / INT32_MAX in the pulse rows; SAMPLES_ACC zero, NaN and negative beside finite and infinite
    extrema: equal on every byte (a NaN is 0x7FF8000000000000 / 0x7FC00000 in both)."""
    rng = np.random.default_rng(257 + masked)
    p = Problem(rng, 257, pad=3, terms_pad=3, off16=masked, masked=masked, restart=True, hostile=True)
    d = OnDevice(p)
    for weights in (ALL_ON, tuple(-w for w in ALL_ON), (1e300, -1e300, 5e-324, 1.0, 1e-310, -1e308, 1.0, 1e308, -1e-320, 3.0),
                    *(alone(k) for k in range(K))):
        d.call(weights)
        d.check((masked, weights))
        if weights is ALL_ON:
            terms, reward = p.view(d.want, "terms_out")[:, :257], p.view(d.want, "reward_out")
            assert np.isnan(terms).any() and np.isinf(terms).any() and np.isnan(reward).any(), "the case holds what it names"
    sig = p.view(p.buf, "sig")
    quiet = (sig[_abi.SIG.SAMPLES_ACC, :257] == 0) & np.isfinite(sig[_abi.SIG.GAP_MIN_ACC, :257]) & (sig[_abi.SIG.GAP_MIN_ACC, :257] < 12.0)
    assert quiet.any(), "SAMPLES_ACC == 0 beside a finite minimum below the floor"


def test_two_shards_in_turn_equal_the_whole_batch():
    """Pointers advanced by 256 environments: the call is elementwise."""
    rng = np.random.default_rng(600)
    for N, pad in ((600, 5), (257, 0)):
        p = Problem(rng, N, pad=pad, terms_pad=pad // 2, masked=True, restart=True)
        whole, shards = OnDevice(p), OnDevice(p)
        whole.call()
        for part in ((0, 256), (256, N - 256)):
            shards.call(part=part)
        whole.check((N, "whole"))
        shards.check((N, "shards"))
        assert shards.dev.cpu().numpy().tobytes() == whole.dev.cpu().numpy().tobytes()


def test_reward_behind_the_gate():
    """257 environments with a mask and restarts; ``pos_before`` is the gated input.  The control is a twin problem reading
    the same ``pos_before`` on the default stream."""
    N = 257
    rng = np.random.default_rng(41)
    p = Problem(rng, N, pad=3, terms_pad=3, masked=True, restart=True)
    before_a = p.view(p.buf, "pos_before").copy()
    before_b = before_a - rng.uniform(1.0, 2.0, N)
    shared = torch.from_numpy(before_a.copy()).to(DEV)
    dev_b = torch.from_numpy(before_b.copy()).to(DEV)
    under, control, warm = OnDevice(p), OnDevice(p), OnDevice(p)

    def call(d):
        desc = p.desc(d.dev.data_ptr())
        desc.pos_before = shared.data_ptr()
        device_reward(desc, DEV)

    call(warm)
    gate = Gate(seconds_on(torch.cuda.default_stream(), lambda: call(warm)))
    want_a, want_b = p.buf.copy(), p.buf.copy()
    p.define(want_a)
    p.view(want_b, "pos_before")[:] = before_b
    p.define(want_b)
    outputs = ("reward_out", "terms_out")
    live = p.view(p.buf, "mask") != 0
    assert live.sum() > 100 and all(p.view(want_a, name).tobytes() != p.view(want_b, name).tobytes() for name in outputs)
    gated(gate, lambda: shared.copy_(dev_b), lambda: call(under), lambda: call(control))
    # the arenas' own `pos_before` blocks hold A and are not read: the expected arenas differ from A's in the outputs only
    p.view(want_b, "pos_before")[:] = before_a
    assert differences(p, under.dev.cpu().numpy(), want_b) == [], "wedm_reward behind the gate"
    got = control.dev.cpu().numpy()
    check_control(all(p.view(got, name).tobytes() == p.view(want_a, name).tobytes() for name in outputs),
                  any(p.view(got, name).tobytes() == p.view(want_b, name).tobytes() for name in outputs), gate, "wedm_reward")


# ------------------------------------------------------------------------------------------------ the stack
def test_the_in_kernel_stack_neither_synchronises_nor_allocates_and_equals_the_oracle_twin():
    """64 x 13, pulse and signal statistics, in-kernel autoreset, every term on, a normaliser and a log, nine control steps:
    every reward, every ``reward_terms`` block and the log's records equal the oracle backend's on every byte; the steps
    after the first run under ``set_sync_debug_mode("error")`` with ``memory_allocated()`` unchanged."""
    steps, runs, reads = 9, {}, {}
    for device in (DEV, "cpu"):
        vec, log, action = in_kernel_stack(device, 1024)
        n = vec.num_envs
        hold = {"reward": torch.zeros((steps, n), dtype=torch.float32, device=device),
                "raw_reward": torch.zeros((steps, n), dtype=torch.float32, device=device),
                "reward_terms": torch.zeros((steps, K, n), dtype=torch.float64, device=device),
                "done": torch.zeros((steps, n), dtype=torch.bool, device=device)}

        def step(i):
            _, scaled, term, trunc, info = vec.step(action)
            hold["reward"][i].copy_(scaled)
            hold["raw_reward"][i].copy_(info["raw_reward"])
            hold["reward_terms"][i].copy_(info["reward_terms"])
            torch.logical_or(term, trunc, out=hold["done"][i])

        step(0)
        allocated = []
        if device == DEV:
            assert vec._shaped._native is not None and log._native is not None
            torch.cuda.synchronize()
            gc.collect()
            gc.disable()
            torch.cuda.set_sync_debug_mode("error")
        try:
            for i in range(1, steps):
                step(i)
                allocated.append(torch.cuda.memory_allocated() if device == DEV else 0)
        finally:
            if device == DEV:
                torch.cuda.set_sync_debug_mode("default")
                gc.enable()
        if device == DEV:
            torch.cuda.synchronize()
            assert allocated[1:] == [allocated[1]] * (steps - 2), allocated
        vec.env.check_errors()
        runs[device], reads[device] = {k: v.cpu() for k, v in hold.items()}, log.read()
        vec.close()
    rc.assert_equal(runs[DEV], runs["cpu"], "what the nine control steps handed out")
    got, want = reads[DEV], reads["cpu"]
    assert list(got) == list(want)
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    terms = runs["cpu"]["reward_terms"]
    assert all(bool((terms[:, k] != 0).any()) for k in range(K)), "every term is at work somewhere in the run"
    assert want["lost"] == 0 and len(want["env"]) > 64 and want["terminated"].any() and want["truncated"].any()
    assert all(np.any(want[f"rw_{name}"] != 0) for name in ("progress", "step", "sparks", "energy", "gap_below"))


def test_a_training_run_with_the_shaped_reward_on_the_gpu_is_the_oracle_backends_run_on_every_byte():
    """The 64 x 13 in-kernel stack of tests/test_policy_net.py's last test with the `ShapedReward` in place of the progress
    reward, nine control steps and two epochs, against the same stack on the oracle backend: every observation, reward and
    flag it hands out, every PPO gradient and ``stats``, the final ``theta``, the log."""
    want_steps, want_calls, want_end, want_log = run_whole("cpu")
    got_steps, got_calls, got_end, got_log = run_whole(DEV)
    assert len(got_steps) == len(want_steps) == rc.K and len(got_calls) == len(want_calls) == 4
    for i, (got, want) in enumerate(zip(got_steps, want_steps)):
        rc.assert_equal(got, want, f"what control step {i + 1} handed out")
    for got, want in zip(got_calls, want_calls):
        rc.assert_equal({n: got[n] for n in ("grad", "stats")}, {n: want[n] for n in ("grad", "stats")}, f"PPO call after step {want['step']}")
    rc.assert_equal({"theta": got_end["net.0"]}, {"theta": want_end["net.0"]}, "theta at the end")
    rc.assert_equal(got_end, want_end, "everything at the end")
    assert any(bool((c["grad"] != 0).any()) for c in want_calls)
    assert list(got_log) == list(want_log) and all(np.asarray(got_log[k]).tobytes() == np.asarray(want_log[k]).tobytes() for k in want_log)
    rewards = torch.stack([s["raw_reward"] for s in want_steps])
    assert len(set(rewards.reshape(-1).tolist())) > 64 and any(np.any(want_log[f"rw_{n}"] != 0) for n in ("shorts", "tmax_above"))
