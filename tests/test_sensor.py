"""`wedm_sensor` on the MI355X (sparc_amd/csrc/wedm_sensor.h): the call against `sensor_reference` on
every byte of an arena that holds all its blocks between guard bands -- ``out``, the ring, ``pos``, ``age``, the padding
columns, the inputs -- over a sequence of twelve calls with restarts and masked environments, at the wave and block edges,
with one and two source planes, 1, 5 and 24 channels, rings of 1, 2 and 8, every stage on, each alone and none, a global id
that wraps, call and episode numbers beyond 2^32; hostile sources and table entries; two shards in turn; the call on a side
stream behind a gate; `Sensor` through `WireEDMVectorEnv` without a host synchronisation or an allocation against its twin on
the CPU oracle backend; and the asymmetric training run on the GPU against the same run on the oracle backend."""
from __future__ import annotations

import gc
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sparc_amd.sensor import device_sensor
from tests import _resume_common as rc
from tests import _sensor_common as sc
from tests._sensor_common import CALLS, T0, WRAP, Problem, differences
from tests._stream_gate import Gate, check_control, gated, seconds_on

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
# (rows per plane, C_out, L, stages, env_id_offset): every value of every factor and every kind of channel set
CASES = (((8,), 1, 1, "all", 0), ((16, 8), 5, 2, "all", WRAP), ((16, 8), 24, 8, "all", 0), ((8,), 24, 8, "mixed", WRAP),
         ((8,), 5, 8, "delay", 0), ((16, 8), 5, 1, "sigma", 0), ((8,), 5, 2, "calib", WRAP), ((16, 8), 1, 2, "lsb", 0),
         ((8,), 5, 1, "clamp", 0), ((16, 8), 24, 2, "identity", WRAP), ((8,), 1, 8, "all", WRAP), ((16, 8), 1, 8, "identity", 0))


class OnDevice:
    """A problem's arena on the device, and its twin on the host that the definition moves on."""

    def __init__(self, p: Problem):
        self.p, self.want = p, p.buf.copy()
        self.dev = torch.from_numpy(p.buf.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    def put(self, blocks) -> None:
        """New contents of input blocks, in both arenas."""
        for name, a in blocks.items():
            self.p.view(self.want, name)[...] = a
            off = self.p.layout[name][0]
            self.dev[off: off + a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()))

    def call(self, t: int, trace=None, **kw) -> None:
        device_sensor(self.p.desc(self.dev.data_ptr(), t, **kw), DEV)
        self.p.define(self.want, t, trace=trace, **kw)

    def check(self, where) -> None:
        assert differences(self.p, self.dev.cpu().numpy(), self.want) == [], where


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_call_against_the_definition_on_every_byte(N):
    """Twelve calls per case; after each the two arenas are equal on every byte.  Call 0 passes ``first``, ``mask`` and
    ``episode`` as NULL in every other case.  Where the channel set has delays, both ``d_eff == d > 0`` and ``d_eff == age <
    d`` occur."""
    rng = np.random.default_rng(7000 + N)
    for i, (planes, C_out, L, kind, offset) in enumerate(CASES):
        p = Problem(rng, N, planes, C_out, L, kind, pad=3 * (i % 2), offset=offset)
        d = OnDevice(p)
        full = short = False
        for call in range(CALLS):
            d.put(sc.sequence_inputs(p, rng, call))
            trace: dict = {}
            given = not (call == 0 and i % 2)
            d.call(T0 + call, trace, first=given, mask=given, episode=given)
            d.check((N, i, call))
            full |= bool(((trace["d_eff"] == trace["delay"]) & (trace["delay"] > 0)).any())
            short |= bool((trace["d_eff"] < trace["delay"]).any())
        if L > 1 and kind in ("all", "delay") and N >= 63:
            assert full and short, (N, i, full, short)


def test_hostile_sources_and_table_entries_at_257_environments():
    """NaNs with payloads, infinities, float32 subnormals and FLT_MAX in the sources; ``lsb`` of 1e-300 and 1e300, ``sigma`` of
    1e300, a negative ``lsb``, ``lo > hi``; ``SOURCE`` and ``MAX_DELAY`` entries far outside their ranges; uninitialised
    ``pos`` / ``age`` under ``first``: equal on every byte, and nothing outside the blocks is touched."""
    rng = np.random.default_rng(257)
    for planes, C_out, L in (((16, 8), 24, 8), ((8,), 13, 2), ((8,), 7, 1)):
        p = Problem(rng, 257, planes, C_out, L, pad=3, offset=WRAP, table=sc.hostile_table(rng, sum(planes), C_out, L))
        d = OnDevice(p)
        for call in range(6):
            new = sc.sequence_inputs(p, rng, call)
            for k, r in enumerate(planes):
                new[f"plane{k}"] = sc.hostile_f32(rng, (r, p.S))
            d.put(new)
            d.call(T0 + call)
            d.check((planes, C_out, L, call))
        out = p.view(d.want, "out")[:, :257]
        assert np.isnan(out).any() and np.isinf(out).any() and (out.view(np.uint32)[np.isnan(out)] == 0x7FC00000).all()
        assert ((out != 0) & (np.abs(out) < np.finfo(np.float32).tiny)).any(), "a subnormal passes through"


def test_two_shards_in_turn_equal_the_whole_batch():
    """Pointers advanced by 256 environments and the offset moved with them: the call is elementwise, the ids are global."""
    rng = np.random.default_rng(600)
    for N, planes, L, offset in ((600, (16, 8), 8, WRAP), (257, (8,), 2, 0)):
        p = Problem(rng, N, planes, 5, L, "all", pad=5, offset=offset)
        whole, shards = OnDevice(p), OnDevice(p)
        for call in range(5):
            new = sc.sequence_inputs(p, rng, call)
            whole.put(new)
            shards.put(new)
            whole.call(T0 + call)
            for part in ((0, 256), (256, N - 256)):
                shards.call(T0 + call, part=part)
            whole.check((N, call, "whole"))
            shards.check((N, call, "shards"))
            assert shards.dev.cpu().numpy().tobytes() == whole.dev.cpu().numpy().tobytes()


def gate_case() -> None:
    """The call on a side stream behind a gate, as tests/_stream_gate.py describes it and tests/test_reward.py uses it: 257
    environments, two planes, a ring of 2; plane 0 is the gated input.  The control is a twin problem reading the same plane
    on the default stream."""
    N = 257
    rng = np.random.default_rng(41)
    p = Problem(rng, N, (16, 8), 5, 2, "all", pad=3)
    a = p.view(p.buf, "plane0").copy()
    b = (a + rng.uniform(1.0, 2.0, a.shape)).astype(np.float32)
    shared = torch.from_numpy(a.copy()).to(DEV)
    dev_b = torch.from_numpy(b.copy()).to(DEV)
    under, control, warm = OnDevice(p), OnDevice(p), OnDevice(p)

    def call(d):
        desc = p.desc(d.dev.data_ptr(), T0)
        desc.plane[0].rows = shared.data_ptr()
        device_sensor(desc, DEV)

    call(warm)
    gate = Gate(seconds_on(torch.cuda.default_stream(), lambda: call(warm)))
    want_a, want_b = p.buf.copy(), p.buf.copy()
    p.define(want_a, T0)
    p.view(want_b, "plane0")[...] = b
    p.define(want_b, T0)
    written = ("out", "ring")
    assert all(p.view(want_a, name).tobytes() != p.view(want_b, name).tobytes() for name in written)
    gated(gate, lambda: shared.copy_(dev_b), lambda: call(under), lambda: call(control))
    # the arenas' own plane 0 holds A and is not read: the expected arenas differ from A's in what is written only
    p.view(want_b, "plane0")[...] = a
    assert differences(p, under.dev.cpu().numpy(), want_b) == [], "wedm_sensor behind the gate"
    got = control.dev.cpu().numpy()
    check_control(all(p.view(got, name).tobytes() == p.view(want_a, name).tobytes() for name in written),
                  any(p.view(got, name).tobytes() == p.view(want_b, name).tobytes() for name in written), gate, "wedm_sensor")


def test_sensor_behind_the_gate():
    """In a process of its own (`python -m tests.test_sensor`), as tests/test_optimizer.py has it.  A gate needs a side stream,
    and the runtime deals its few hardware queues to the streams of a process as they are first used: a stream taken here
    would move every later module's gate to another queue, and the one that comes to share the default stream's cannot hold
    its control back.  The child's side stream is the first of its process and gets a queue of its own."""
    run = subprocess.run([sys.executable, "-m", "tests.test_sensor"], cwd=str(ROOT), capture_output=True, text=True)
    assert run.returncode == 0 and "gate case ok" in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the stack
def test_the_in_kernel_stack_neither_synchronises_nor_allocates_and_equals_the_oracle_twin():
    """64 x 13, pulse and signal columns, the wire profile, in-kernel autoreset, a sensor with noise, calibration and delays,
    a normaliser, the shaped reward and a log, nine control steps: every observation, raw observation, reward and flag, the
    sensor's state and the log's records equal the oracle backend's on every byte; the steps after the first run under
    ``set_sync_debug_mode("error")`` with ``memory_allocated()`` unchanged."""
    steps, runs, reads, held = 9, {}, {}, {}
    for device in (DEV, "cpu"):
        vec, log, action = sc.in_kernel_stack(device, 1024)
        n, D = vec.num_envs, len(vec.obs_names)
        hold = {"obs": torch.zeros((steps, n, D), dtype=torch.float32, device=device),
                "raw": torch.zeros((steps, n, len(vec.raw_obs_names)), dtype=torch.float32, device=device),
                "reward": torch.zeros((steps, n), dtype=torch.float32, device=device),
                "done": torch.zeros((steps, n), dtype=torch.bool, device=device)}

        def step(i):
            obs, scaled, term, trunc, info = vec.step(action)
            hold["obs"][i].copy_(obs)
            hold["raw"][i].copy_(info["raw_observation"])
            hold["reward"][i].copy_(scaled)
            torch.logical_or(term, trunc, out=hold["done"][i])

        step(0)
        allocated = []
        if device == DEV:
            assert vec.sensor._native is not None and log._native is not None
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
        runs[device], reads[device], held[device] = {k: v.cpu() for k, v in hold.items()}, log.read(), sc.sensor_blocks(vec.sensor)
        vec.close()
    rc.assert_equal(runs[DEV], runs["cpu"], "what the nine control steps handed out")
    rc.assert_equal(held[DEV], held["cpu"], "the sensor's state")
    got, want = reads[DEV], reads["cpu"]
    assert list(got) == list(want) and all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want)
    assert bool(runs["cpu"]["done"].any()) and len(set(held["cpu"]["sensor.age"].tolist())) > 1
    assert not torch.equal(runs["cpu"]["obs"][:, :, 1], runs["cpu"]["obs"][:, :, 12]), "the measured voltage is not the clean one"


def test_an_asymmetric_training_run_on_the_gpu_is_the_oracle_backends_run_on_every_byte(tmp_path):
    """An actor `PolicyNet` on the measured columns and a critic `PolicyNet` on all columns, both reading the rollout in place,
    two `Adam`s, nine control steps and two epochs: both ``theta``s, the optimisers' moments and the sensor's state agree with
    the oracle backend's run with the NumPy definitions on every byte, and the run cut once and resumed is the same."""
    ends = {}
    for device in ("cpu", DEV):
        st = sc.AsymmetricStack(device, rc.RUN_SEEDS)
        try:
            st.run(5)
            st.save(tmp_path / f"{device.replace(':', '')}.pt")
            st.run(rc.K)
            ends[device] = st.everything()
        finally:
            st.close()
    rc.assert_equal(ends[DEV], ends["cpu"], "everything at the end")
    other = sc.AsymmetricStack(DEV, rc.OTHER_SEEDS)
    try:
        other.run(2)
        other.load(tmp_path / "cuda0.pt")
        other.run(rc.K)
        rc.assert_equal(other.everything(), ends[DEV], "cut after control step 5 and resumed")
    finally:
        other.close()
    fresh = sc.AsymmetricStack("cpu", rc.RUN_SEEDS)
    try:
        start = fresh.everything()
    finally:
        fresh.close()
    assert all(not torch.equal(start[k], ends["cpu"][k]) for k in ("actor.theta", "critic.theta", "actor.m", "critic.v", "sensor.ring"))


if __name__ == "__main__":
    gate_case()
    print("gate case ok")
