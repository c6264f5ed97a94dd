"""The seeded minibatch permutation on the MI355X (sparc_amd/csrc/wedm_minibatch.h, sparc_amd/minibatch.py, DESIGN.md section
4.24): `wedm_minibatch_index` against `minibatch_index_reference` on every byte of one arena per block -- guard bands,
``valid`` left alone, ``index``, ``count``, both workspaces -- at the wave, tile and pass edges, for every kind of mask, with
``valid`` and ``index`` off their natural boundaries, in one call and in three; repeats; an epoch without a host
synchronisation or an allocation; the call on a side stream behind a gate; and a whole training run on the GPU against the
same run on the oracle backend, every drawn index included."""
from __future__ import annotations

import ctypes as C
import gc
import itertools
import subprocess
import sys
from pathlib import Path
from typing import Optional

import numpy as np
import pytest
import torch

from sparc_amd import Adam, MinibatchSampler, _abi, _lib
from sparc_amd.minibatch import minibatch_index_reference
from sparc_amd.optimizer import SKIPPED_KL, T
from tests import _minibatch_common as mc
from tests import _resume_common as rc
from tests._arena import FILL, Arena
from tests._normalize_common import same_bits
from tests._stream_gate import Gate, check_control, gated, seconds_on
from tests.test_policy_net import _stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
SMALL = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
SIZES = SMALL + (65537, 1048577)   # the last: the first size whose tile scan takes more than one pass
BLOCKS = ("valid", "index", "count", "tile_counts", "tile_base")
FORMS = {"one call": (0,), "three calls": (_abi.MB_COUNT, _abi.MB_OFFSETS, _abi.MB_SCATTER)}
# (bytes of valid past a 4-byte boundary, whether index lies 8 bytes past a 16-byte boundary, form)
LAYOUTS = tuple(itertools.product((0, 1, 3), (False, True), tuple(FORMS)))


def device_call(desc) -> None:
    _lib.call_stateless(_lib.load().wedm_minibatch_index, torch.device(DEV), C.byref(desc))


class Problem:
    """The blocks of one call on the device, each inside an arena of 0xA5 bytes (tests/_arena.py): ``valid`` ``valid_shift``
    bytes past a 16-byte boundary (None: the call gets NULL and the arena stays as it is), ``index`` 8 bytes past one where
    ``index_shift``."""

    def __init__(self, R: int, valid: Optional[np.ndarray], valid_shift: int = 0, index_shift: bool = False):
        self.R, self.tiles, self.null = R, -(-R // 1024), valid is None
        host = {"valid": np.ones(R, dtype=np.uint8) if valid is None else valid, "index": np.empty(R, dtype=np.int64),
                "count": np.empty(2, dtype=np.int64), "tile_counts": np.empty(self.tiles, dtype=np.int32),
                "tile_base": np.empty(self.tiles, dtype=np.int32)}
        lead = {"valid": valid_shift, "index": int(index_shift)}
        self.arena, self.view, self.lead = {}, {}, {}
        for name in BLOCKS:
            a = host[name]
            like = torch.empty((1, lead.get(name, 0) + a.shape[0]), dtype=torch.from_numpy(a).dtype, device=DEV)
            self.arena[name] = arena = Arena(name, like, like.shape[1], like.shape[1])
            self.lead[name], self.view[name] = lead.get(name, 0), arena.view[0, lead.get(name, 0):]
        self.view["valid"].copy_(torch.from_numpy(host["valid"]))
        torch.cuda.synchronize()
        self.image = {name: self.arena[name].raw.cpu().numpy().copy() for name in BLOCKS}   # every byte, bands included
        assert self.view["valid"].data_ptr() % 4 == valid_shift % 4 and self.view["index"].data_ptr() % 16 == 8 * int(index_shift)

    def expect(self, name: str, host: np.ndarray) -> None:
        arena = self.arena[name]
        at = (arena.lead + self.lead[name]) * arena.itemsize
        self.image[name][at: at + host.nbytes] = host.view(np.uint8)

    def desc(self, flags: int, n: int, seed: int, draw: int):
        v = self.view
        return _abi.MbDesc(valid=None if self.null else v["valid"].data_ptr(), index=v["index"].data_ptr(), count=v["count"].data_ptr(),
                           tile_counts=v["tile_counts"].data_ptr(), tile_base=v["tile_base"].data_ptr(), seed=seed, draw=draw,
                           rows=self.R, n_parts=n, flags=flags)

    def differing(self) -> list:
        torch.cuda.synchronize()
        return [name for name in BLOCKS if not np.array_equal(self.arena[name].raw.cpu().numpy(), self.image[name])]


def _check(R: int, name: str, valid: Optional[np.ndarray], n: int, layout, seed: int, draw: int) -> None:
    valid_shift, index_shift, form = layout
    p = Problem(R, valid, valid_shift, index_shift)
    want = minibatch_index_reference(valid, n, seed, draw, rows=R)
    for block, host in zip(BLOCKS[1:], want):
        p.expect(block, host)
    for flags in FORMS[form]:
        device_call(p.desc(flags, n, seed, draw))
    assert p.differing() == [], (R, name, n, layout)


@pytest.mark.parametrize("R", SIZES)
def test_the_call_is_the_definition_on_every_byte(R):
    """Every mask of `tests._minibatch_common.masks` with every number of parts (at the two large sizes one per mask, in
    turn), the layouts and forms in turn: every size sees every layout in both forms."""
    layouts = itertools.cycle(LAYOUTS)
    most = min(R, _abi.MB_MAX_PARTS)   # as many parts as rows, where the call takes that many
    parts = sorted({n for n in ((1, 2, 7, 8, most) if R in SMALL else (1, 2, 7, 8)) if n <= most})
    turn = itertools.cycle(parts)
    seen = set()
    for name, valid in mc.masks(R, seed=R).items():
        for n in (parts if R in SMALL else (next(turn), next(turn))):
            layout = next(layouts)
            seen.add(layout)
            _check(R, name, valid, n, layout, seed=0x9E3779B97F4A7C15 ^ R, draw=2 ** 32 + n)
    if R > 2:
        assert len(seen) == len(LAYOUTS), len(seen)


def test_the_same_call_twice_from_the_same_start_gives_the_same_bytes():
    R, n = 65537, 7
    valid = mc.masks(R, seed=1)["most"]
    outs = []
    for _ in range(2):
        p = Problem(R, valid, 3, True)
        device_call(p.desc(0, n, 77, 9))
        torch.cuda.synchronize()
        outs.append({k: p.arena[k].raw.clone() for k in BLOCKS})
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in BLOCKS)
    # and a second call over the blocks the first one filled changes none of their bytes
    before = {k: p.arena[k].raw.clone() for k in BLOCKS}
    device_call(p.desc(0, n, 77, 9))
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], p.arena[k].raw) for k in BLOCKS)
    mc.check_placement(p.view["index"].cpu().numpy(), valid, n)


def test_an_epoch_neither_synchronises_nor_allocates():
    vec, head, ppo, buf, net = _stack()
    opt = Adam(net, lr=lambda k: 1e-3 / (1 + k), max_grad_norm=0.5, kl_limit=0.02)
    sampler = MinibatchSampler(buf, 2, seed=5)
    assert opt._native is not None and sampler._native is not None

    def update():
        opt.begin_update()
        for idx in sampler.draw():
            opt.zero_grad()
            params, value = net(rollout=buf, index=idx)
            stats = ppo.backward(params, value, rollout=buf, index=idx)
            opt.step(stats)
            del params, value, stats

    update()   # buffers grow to their sizes
    torch.cuda.synchronize()
    first = sampler.index.clone()
    theta = net.theta.detach().clone()
    gc.collect()
    gc.disable()
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        update()
        after = torch.cuda.memory_allocated()
        assert after == before, (before, after)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    valid = buf.computed["valid"]
    assert sampler.draws == 2 and not same_bits(theta, net.theta) and float(opt.state[T] + opt.state[SKIPPED_KL]) == 4.0
    for d, got in ((0, first), (1, sampler.index)):
        want = sampler.expected(valid, d)
        assert np.array_equal(got.cpu().numpy(), want[0])
    assert sampler.count.tolist() == want[1].tolist() and not torch.equal(first, sampler.index)
    gathered = list(buf.minibatches(2, sampler=sampler))
    assert torch.equal(torch.cat([g["reward"] for g in gathered]), buf.flat()["reward"][sampler.index]) and sampler.draws == 3
    vec.close()


GATE_SIZES = (1025, 1048577)   # one pass of the tile scan, and two


def gate_case(R: int) -> None:
    """The call on a side stream behind a gate, as tests/_stream_gate.py describes it; ``valid`` is the gated input."""
    n, seed, draw = 8, 21, 3
    all_masks = mc.masks(R, seed=2)
    va, vb = all_masks["most"], all_masks["power of two"]
    want_a, want_b = (minibatch_index_reference(v, n, seed, draw) for v in (va, vb))
    p, control, warm = Problem(R, va), Problem(R, va), Problem(R, va)
    device_call(warm.desc(0, n, seed, draw))   # warm-up: the code is loaded
    gate = Gate(seconds_on(torch.cuda.current_stream(), lambda: device_call(warm.desc(0, n, seed, draw))))
    vb_dev = torch.from_numpy(vb).to(DEV)
    cdesc = control.desc(0, n, seed, draw)
    cdesc.valid = p.desc(0, n, seed, draw).valid   # the control reads the same valid block
    gated(gate, lambda: p.view["valid"].copy_(vb_dev, non_blocking=True), lambda: device_call(p.desc(0, n, seed, draw)),
          lambda: device_call(cdesc))
    got = [control.view[k].cpu().numpy() for k in BLOCKS[1:]]
    check_control(all(np.array_equal(g, w) for g, w in zip(got, want_a)), all(np.array_equal(g, w) for g, w in zip(got, want_b)), gate,
                  "wedm_minibatch_index")
    assert all(np.array_equal(p.view[k].cpu().numpy(), w) for k, w in zip(BLOCKS[1:], want_b))


def test_the_call_runs_on_the_current_stream_behind_a_gate():
    """In a process of its own (`python -m tests.test_minibatch`), as tests/test_optimizer.py runs its gate: a side stream
    taken inside the session would move later modules' gates onto the default stream's hardware queue."""
    run = subprocess.run([sys.executable, "-m", "tests.test_minibatch"], cwd=str(ROOT), capture_output=True, text=True)
    assert run.returncode == 0 and f"gate cases ok: {len(GATE_SIZES)}" in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])


def test_a_training_run_on_the_gpu_is_the_oracle_backends_run_on_every_byte():
    """The 64 x 13 in-kernel stack with `PolicyNet`, `Adam` and a `MinibatchSampler` on the GPU, nine control steps and two
    epochs, against the same stack on the oracle backend: every observation, reward and flag it hands out, every drawn index,
    every PPO gradient, ``stats`` and ``info``, and ``theta``, ``m``, ``v``, ``state`` and the sampler's blocks at the end.  No
    tensor that the host made enters an epoch."""
    want_steps, want_calls, want_end = mc.run_whole("in-kernel", "cpu")
    got_steps, got_calls, got_end = mc.run_whole("in-kernel", DEV)
    assert len(got_steps) == len(want_steps) == rc.K and len(want_calls) == 4
    for i, (got, want) in enumerate(zip(got_steps, want_steps)):
        rc.assert_equal(got, want, f"what control step {i + 1} handed out")
    mc.assert_calls_equal(got_calls, want_calls, "GPU against the oracle backend")
    names = ("net.0", "opt.m", "opt.v", "opt.state", "opt.calls", "mb.index", "mb.count", "mb.seed_parts_draws")
    rc.assert_equal({n: got_end[n] for n in names}, {n: want_end[n] for n in names}, "theta, m, v, state and the sampler at the end")


if __name__ == "__main__":
    for size in GATE_SIZES:
        gate_case(size)
    print(f"gate cases ok: {len(GATE_SIZES)}")
