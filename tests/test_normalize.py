"""Running normalisation on the MI355X (sparc_amd/csrc/wedm_normalize.h, sparc_amd/normalize.py):
`wedm_normalize` against `torch_normalize` on every byte of everything it writes -- statistics, tile partials, outputs and
per-environment rows -- at the wave, block and tile edges, with its blocks in guard bands; shards reduced and applied in turn
against the whole batch; and through `WireEDMVectorEnv`, without a host synchronisation or an allocation per step."""
from __future__ import annotations

import gc
import math

import numpy as np
import pytest
import torch

from sparc_amd import Normalizer, WireEDMVectorEnv, _abi
from sparc_amd.normalize import APPLY, REDUCE, ROW_NAMES, ROWS, STEP, UPDATE, device_normalize, fresh_stats, torch_normalize
from tests._gae_common import is_subnormal
from tests._normalize_common import columns, same_bits
from tests._snapshot_common import assert_same, everything, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, BAND = 0xA5, 4096


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
    """One batch of synthetic blocks on the device and the host: planes of the column kinds with NaN in the padding columns
    ``[num_envs, stride)``, rewards, dones, and everything the call writes.  `call` runs `wedm_normalize`, `expect` the host
    definition on the same data; both advance the same running state."""

    def __init__(self, N, D, seed, split=None, pad=5, use_mask=True, use_skip=True, clips=(10.0, 10.0), gamma=0.99, eps=1e-8,
                 n_tiles_total=None):
        self.N, self.D, self.C = N, D, D + 1
        self.rng = np.random.default_rng(seed)
        self.rows_n = (D,) if not split else (split, D - split)
        self.strides = tuple(N + pad + 3 * k for k in range(len(self.rows_n)))
        self.use_mask, self.use_skip = use_mask, use_skip
        self.kw = dict(gamma=gamma, eps=eps, clip_obs=clips[0], clip_reward=clips[1])
        self.tiles = -(-N // 256)
        self.n_tiles_total = self.tiles if n_tiles_total is None else n_tiles_total
        self.skip_h = (self.rng.random(D) < 0.3).astype(np.uint8) if use_skip else None
        self.skip = Banded(self.skip_h) if use_skip else None
        self.stats_h = fresh_stats(self.C)
        self.stats = [Banded(self.stats_h), Banded(poisoned((3, self.C), np.float64))]
        self.cur = 0
        self.rows_h = {name: (self.rng.integers(0, 5, N).astype(dt) if name != "finished" else np.zeros(N, dt)) for name, dt in ROWS}
        self.rows = {name: Banded(v) for name, v in self.rows_h.items()}
        self.partials_h = poisoned((self.n_tiles_total, 3, self.C), np.float64)
        self.partials = Banded(self.partials_h)
        self.obs_out = Banded(poisoned((N, D), np.float32))
        self.reward_out = Banded(poisoned((N,), np.float32))
        self.draw()

    def draw(self, mask=None):
        N, rng = self.N, self.rng
        x = columns(rng, N, self.D)
        self.planes_h, lo = [], 0
        for n_rows, stride in zip(self.rows_n, self.strides):
            block = np.full((n_rows, stride), np.nan, dtype=np.float32)
            block[:, :N] = x[lo: lo + n_rows]
            self.planes_h.append(block)
            lo += n_rows
        self.reward_h = rng.normal(size=N).astype(np.float32)
        self.term_h, self.trunc_h = rng.random(N) < 0.1, rng.random(N) < 0.1
        self.mask_h = (rng.random(N) >= 0.2 if mask is None else mask) if self.use_mask else None
        self.planes = [Banded(b) for b in self.planes_h]
        self.reward, self.term, self.trunc = Banded(self.reward_h), Banded(self.term_h), Banded(self.trunc_h)
        self.mask = Banded(self.mask_h) if self.mask_h is not None else None

    def inputs(self):
        out = {f"plane{k}": p for k, p in enumerate(self.planes)}
        out.update(reward=self.reward, terminated=self.term, truncated=self.trunc, stats_in=self.stats[self.cur])
        if self.mask is not None:
            out["mask"] = self.mask
        if self.skip is not None:
            out["skip"] = self.skip
        return out

    def blocks(self):
        out = dict(self.inputs(), stats_out=self.stats[1 - self.cur], partials=self.partials, obs_out=self.obs_out,
                   reward_out=self.reward_out)
        out.update(self.rows)
        return out

    def desc(self, flags, lo=0, count=None, tile_offset=0):
        """The descriptor of environments [lo, lo + count): a shard is the same blocks entered ``lo`` elements further on."""
        count = self.N - lo if count is None else count
        at = lambda b, scale=1: None if b is None else b.t.data_ptr() + lo * scale * b.t.element_size()
        d = _abi.NormDesc(
            reward=at(self.reward), terminated=at(self.term), truncated=at(self.trunc), mask=at(self.mask),
            skip=None if self.skip is None else self.skip.t.data_ptr(), obs_out=at(self.obs_out, self.D), reward_out=at(self.reward_out),
            stats_in=self.stats[self.cur].t.data_ptr(), stats_out=self.stats[1 - self.cur].t.data_ptr(),
            partials=self.partials.t.data_ptr(), tile_offset=tile_offset, n_tiles_total=self.n_tiles_total, flags=flags,
            num_envs=count, **{name: at(b) for name, b in self.rows.items()},
            **self.kw)
        for k, p in enumerate(self.planes):
            d.plane[k].rows, d.plane[k].n_rows, d.plane[k].stride = at(p), p.t.shape[0], p.t.shape[1]
        return d

    def call(self, flags, **kw):
        device_normalize(self.desc(flags, **kw), DEV)

    def expect(self, flags):
        """The host definition on the whole batch; takes over the statistics, the partials and the rows."""
        step = bool(flags & STEP)
        out = torch_normalize(self.planes_h, self.N, self.stats_h, reward=self.reward_h, terminated=self.term_h,
                              truncated=self.trunc_h, mask=self.mask_h, skip=self.skip_h, rows=self.rows_h,
                              partials=self.partials_h, n_tiles_total=self.n_tiles_total, flags=flags, **self.kw)
        self.stats_h, self.partials_h = out["stats_out"].numpy(), out["partials"].numpy()
        self.rows_h = {name: out[name].numpy() for name in ROW_NAMES}
        self.obs_h = out["obs_out"].numpy()
        if step:
            self.reward_out_h = out["reward_out"].numpy()
        return out

    def flip(self):
        self.cur = 1 - self.cur

    def differences(self, step=True):
        """Names of the written blocks whose bytes differ from the host's (after `call`, `expect` and `flip`)."""
        torch.cuda.synchronize()
        pairs = dict(stats_out=(self.stats[self.cur].t, self.stats_h), partials=(self.partials.t, self.partials_h),
                     obs_out=(self.obs_out.t, self.obs_h))
        if step:
            pairs["reward_out"] = (self.reward_out.t, self.reward_out_h)
        pairs.update({name: (self.rows[name].t, self.rows_h[name]) for name in ROW_NAMES})
        return [name for name, (got, want) in pairs.items() if not same_bits(got, want)]


# ------------------------------------------------------------------------------------------------ the call on synthetic planes
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
WIDTHS = (1, 8, 16, 159)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("N", SIZES)
def test_five_calls_equal_the_definition_on_every_byte(N, D):
    """The wave (64), block and tile (256) edges by every width; one plane or two (strides past num_envs, each its own);
    mask, skip and finite clips switched by the case, so that every combination occurs; five consecutive step calls with
    the statistics buffers alternating, the third of them in evaluation mode and the second without a mask."""
    case = SIZES.index(N) * len(WIDTHS) + WIDTHS.index(D)
    split = None if D == 1 or case % 2 == 0 else max(1, D // 3)
    clips = (10.0, 10.0) if case & 4 else (math.inf, math.inf)
    p = Problem(N, D, seed=case, split=split, use_mask=bool(case & 1) or D == 8, use_skip=bool(case & 2) or D == 16, clips=clips)
    for k in range(5):
        if k:
            p.draw()
        if k == 1 and p.use_mask:
            p.mask_h, p.mask = None, None
        flags = STEP if k == 2 else UPDATE | STEP
        before = {name: b.t.clone() for name, b in p.inputs().items()}
        p.call(flags)
        p.expect(flags)
        blocks = p.blocks()
        p.flip()
        assert p.differences() == [], (N, D, k)
        assert all(same_bits(blocks[name].t, t) for name, t in before.items()), "an input was written"
        assert [name for name, b in blocks.items() if not b.bands_intact()] == []
    assert p.stats_h[0, 0] > 1e-4 and (N == 1 or p.rows_h["finished"].any())   # (one environment may well finish nothing)


def test_observation_only_call_as_after_a_reset():
    p = Problem(300, 20, seed=40, split=8)
    rows = {name: b.t.clone() for name, b in p.rows.items()}
    p.call(UPDATE)
    out = p.expect(UPDATE)
    p.flip()
    assert p.differences(step=False) == []
    assert all(same_bits(p.rows[name].t, rows[name]) for name in ROW_NAMES)                   # no episode accounting
    assert bool((p.reward_out.raw == FILL).all())                                              # no reward is written
    assert out["stats_out"][:, 20].tolist() == [1e-4, 0.0, 1e-4]                               # the return's column passes through


def test_an_empty_batch_writes_the_outputs_and_nothing_else():
    p = Problem(300, 9, seed=41)
    p.draw(mask=np.zeros(300, dtype=bool))
    rows = {name: b.t.clone() for name, b in p.rows.items()}
    p.call(UPDATE | STEP)
    p.expect(UPDATE | STEP)
    p.flip()
    assert p.differences() == []
    assert same_bits(p.stats[0].t, p.stats[1].t)                                               # stats_out == stats_in
    assert all(same_bits(p.rows[name].t, rows[name]) for name in ROW_NAMES)                   # the rows are untouched
    assert not bool((p.obs_out.t.view(torch.uint8) == FILL).all(dim=-1).any())                 # the outputs are written
    assert not bool((p.reward_out.t.view(torch.uint8).view(-1, 4) == FILL).all(dim=-1).any())


def test_run_twice_gives_the_same_bits():
    got = []
    for _ in range(2):
        p = Problem(1000, 16, seed=42, split=5)
        p.call(UPDATE | STEP)
        torch.cuda.synchronize()
        got.append({name: b.t.clone() for name, b in p.blocks().items()})
    assert all(same_bits(got[0][name], got[1][name]) for name in got[0])


def test_float32_subnormals_are_kept_on_input_and_output():
    """Three columns of its own planes, 300 environments: 1e-41 x N(0,1) (float32 subnormals on input, and around the
    smallest normal on output); 1e-33 x N(0,1) on running statistics of variance 1e12, so that the standardised output, 1e-39,
    is a float32 subnormal made from normal inputs; and a unit normal.  The definition (NumPy, which keeps subnormals on
    load and on the float64 -> float32 store) and the call agree on every byte: statistics, partials, outputs and rows."""
    p = Problem(300, 3, seed=46, use_skip=False, clips=(math.inf, math.inf))
    rng = np.random.default_rng(460)
    x = np.stack([1e-41 * rng.normal(size=300), 1e-33 * rng.normal(size=300), rng.normal(size=300)]).astype(np.float32)
    p.planes_h[0][:, :300] = x
    p.planes[0].t.copy_(torch.from_numpy(p.planes_h[0]))
    p.stats_h[:, 1] = [100.0, 0.0, 100.0 * 1e12]
    p.stats[0].t.copy_(torch.from_numpy(p.stats_h))
    assert is_subnormal(x[0]).all() and not is_subnormal(x[1:]).any()
    p.call(UPDATE | STEP)
    p.expect(UPDATE | STEP)
    blocks = p.blocks()
    p.flip()
    assert p.differences() == []
    assert [name for name, b in blocks.items() if not b.bands_intact()] == []
    out = is_subnormal(p.obs_h)
    assert out[:, 0].sum() >= 50 and (~out[:, 0] & (p.obs_h[:, 0] != 0.0)).sum() >= 50, "column 0: outputs on either side of the smallest normal"
    assert out[:, 1].sum() >= 250 and not out[:, 2].any() and p.stats_h[1, 0] != 0.0 and abs(p.stats_h[1, 0]) < 1e-41


# ------------------------------------------------------------------------------------------------ shards in turn
@pytest.mark.parametrize("shards", [4, 2])
def test_shards_reduced_and_applied_in_turn_equal_the_whole_batch(shards):
    """1 024 environments as one call, and as ``shards`` shards that each REDUCE into their tiles of one shared workspace and
    then each APPLY: what an all-gather of the partials between the two phases gives several devices."""
    whole = Problem(1024, 12, seed=43, split=8)
    whole.call(UPDATE | STEP)
    whole.expect(UPDATE | STEP)
    whole.flip()
    assert whole.differences() == []
    parts = Problem(1024, 12, seed=43, split=8)
    size = 1024 // shards
    for s in range(shards):
        parts.call(UPDATE | STEP | REDUCE, lo=s * size, count=size, tile_offset=s * size // 256)
    for s in range(shards):
        parts.call(UPDATE | STEP | APPLY, lo=s * size, count=size, tile_offset=s * size // 256)
    torch.cuda.synchronize()
    a, b = whole.blocks(), parts.blocks()
    for name in ("partials", "obs_out", "reward_out") + ROW_NAMES:
        assert same_bits(a[name].t, b[name].t), name
    assert same_bits(whole.stats[whole.cur].t, parts.stats[1 - parts.cur].t)
    assert [name for name, blk in b.items() if not blk.bands_intact()] == []


@pytest.mark.parametrize("n_tiles_total", [256, 257, 1000, 1025, 4096])
def test_the_fold_of_a_large_workspace(n_tiles_total):
    """The fold gives a lane 1, 2, 4, 8 or 16 tiles, by the size of the workspace: each of them against the host's tree, on a
    workspace of other shards' nodes (a third of them EMPTY) around this batch's two tiles."""
    p = Problem(300, 3, seed=45, n_tiles_total=n_tiles_total)
    rng = np.random.default_rng(n_tiles_total)
    nodes = np.stack([rng.integers(1, 257, (n_tiles_total, 4)).astype(np.float64), rng.normal(size=(n_tiles_total, 4)),
                      rng.uniform(0.0, 50.0, (n_tiles_total, 4))], axis=1)
    nodes[rng.random(n_tiles_total) < 0.33] = 0.0
    p.partials_h = nodes
    p.partials.t.copy_(torch.from_numpy(nodes))
    offset = n_tiles_total - 2
    p.call(UPDATE | STEP | REDUCE, tile_offset=offset)
    p.call(UPDATE | STEP | APPLY, tile_offset=offset)
    out = torch_normalize(p.planes_h, p.N, p.stats_h, reward=p.reward_h, terminated=p.term_h, truncated=p.trunc_h, mask=p.mask_h,
                          skip=p.skip_h, rows=p.rows_h, partials=nodes, tile_offset=offset, n_tiles_total=n_tiles_total, **p.kw)
    torch.cuda.synchronize()
    assert same_bits(p.partials.t, out["partials"]) and same_bits(p.stats[1].t, out["stats_out"])
    assert same_bits(p.obs_out.t, out["obs_out"]) and same_bits(p.reward_out.t, out["reward_out"])
    assert [name for name, b in p.blocks().items() if not b.bands_intact()] == []


# ------------------------------------------------------------------------------------------------ guard bands
def test_every_block_in_guard_bands_and_inputs_and_padding_unchanged():
    """The widest call (159 columns over two planes, three tiles, the last one short, strides past num_envs, a workspace
    with room past this batch's tiles): the bands of every block, every input byte -- the planes' padding columns
    ``[num_envs, stride)`` among them -- and the workspace's other tiles are as they were."""
    p = Problem(600, 159, seed=44, split=16, pad=9, n_tiles_total=5)
    before = {name: b.t.clone() for name, b in p.inputs().items()}
    tail = p.partials.t[3:].clone()
    d = p.desc(UPDATE | STEP | REDUCE, tile_offset=0)
    device_normalize(d, DEV)
    torch.cuda.synchronize()
    blocks = p.blocks()
    assert [name for name, b in blocks.items() if not b.bands_intact()] == []
    assert same_bits(p.partials.t[3:], tail) and bool((tail.view(torch.uint8) == FILL).all())
    p.partials.t[3:] = 0.0                                 # EMPTY: the tiles of shards that hold nothing
    p.partials_h[3:] = 0.0
    p.call(UPDATE | STEP | APPLY)
    torch.cuda.synchronize()
    p.expect(UPDATE | STEP)
    p.flip()
    assert p.differences() == []
    assert [name for name, b in blocks.items() if not b.bands_intact()] == []
    assert all(same_bits(blocks[name].t, t) for name, t in before.items())
    for k, plane in enumerate(p.planes):
        assert bool(torch.isnan(plane.t[:, p.N:]).all()), f"plane {k}: padding columns"


# ------------------------------------------------------------------------------------------------ through the adapter
def _pair(n, bins, opts):
    kw = {} if bins is None else dict(wire_profile_bins=bins)
    plain = WireEDMVectorEnv(make(DEV, n, "autoreset", "s128", **opts), max_episode_steps=4000, **kw)
    norm = Normalizer()
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s128", **opts), max_episode_steps=4000, normalizer=norm, **kw)
    return plain, vec, norm


def _kept(info):
    """A step's info with every tensor cloned (the episode statistics are the normaliser's live rows)."""
    return {k: (_kept(v) if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v) for k, v in info.items()}


@pytest.mark.parametrize("bins,opts", [(None, {}), (8, dict(pulse_stats=True, signal_stats=True))], ids=["plain", "profile-stats"])
def test_adapter_equals_the_definition_step_by_step(bins, opts):
    n = 300
    plain, vec, norm = _pair(n, bins, opts)
    D = len(vec.obs_names)
    assert D == (8 if bins is None else 16 + 4 + 2 * bins)
    skip = np.array([name == "spark_state" for name in vec.obs_names], dtype=np.uint8)
    stats, rows = fresh_stats(D + 1), {name: np.zeros(n, dtype=dt) for name, dt in ROWS}
    outs, finished = [], np.zeros(n, dtype=bool)
    for v in (plain, vec):
        obs, info = v.reset(seed=21)
        v.env.state.workpiece_position = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=DEV)
        v.env.state.wire_position = 10.0
        outs.append([(obs.clone(), info)])
    for i in range(10):
        for v, o in zip((plain, vec), outs):
            if i in (1, 5):   # the launch's in-kernel autoreset takes them
                v.env.state.done[::7] = True
            ob, r, te, tr, info = v.step(v.env.make_action(0.1, 80.0, 9, 3.0, 30.0))
            o.append((ob.clone(), r.clone(), te.clone(), tr.clone(), _kept(info)))
    torch.cuda.synchronize()
    for k, (p, g) in enumerate(zip(*outs)):
        planes = [np.ascontiguousarray(p[0].cpu().numpy().T)]
        assert same_bits(g[-1]["raw_observation"], p[0]), k
        if k == 0:
            want = torch_normalize(planes, n, stats, skip=skip, flags=UPDATE)
        else:
            want = torch_normalize(planes, n, stats, reward=p[1], terminated=p[2], truncated=p[3], skip=skip, rows=rows)
            rows = {name: want[name].numpy() for name in ROW_NAMES}
            finished |= rows["finished"].astype(bool)
            assert same_bits(g[1], want["reward_out"]) and same_bits(g[4]["raw_reward"], p[1]), k
            assert torch.equal(g[2], p[2]) and torch.equal(g[3], p[3]) and torch.equal(g[4]["episode"], p[4]["episode"])
            es = g[4]["episode_stats"]
            assert same_bits(es["r"], want["last_return"]) and same_bits(es["l"], want["last_length"]), k
            assert same_bits(es["count"], want["ep_count"]) and same_bits(es["finished"], want["finished"]), k
        assert same_bits(g[0], want["obs_out"]), k
        stats = want["stats_out"].numpy()
    assert same_bits(norm.stats, torch.from_numpy(stats))
    assert all(same_bits(norm.rows[name], rows[name]) for name in ROW_NAMES)
    assert rows["ep_count"].max() >= 2 and finished.any() and len(set(rows["ep_length"].tolist())) > 1
    assert any(float(p[1].abs().sum()) > 0 for p in outs[0][1:])
    # the physics is the plain adapter's, on every block
    assert_same(everything(vec.env), everything(plain.env), "physics state")
    # fork carries the rows
    norm.rows["ep_return"][:4] = torch.tensor([1.5, 2.5, 3.5, 4.5], dtype=torch.float64, device=DEV)
    src, dst = [0, 1, 3], [200, 201, 299]
    vec.fork(src, dst)
    for t in norm.rows.values():
        assert torch.equal(t[dst], t[src])
    assert norm.rows["ep_return"][299].item() == 4.5


def test_steps_with_a_normalizer_neither_synchronise_nor_allocate():
    env = make(DEV, 4096, "autoreset", "s128")
    vec = WireEDMVectorEnv(env, max_episode_steps=3000, normalizer=Normalizer(), wire_profile_bins=8)
    vec.reset(seed=5)
    env.state.workpiece_position = torch.linspace(10.4, 25.0, 4096, dtype=torch.float64, device=DEV)
    env.state.wire_position = 10.0
    act = env.make_action(0.05, 80.0, 13, 2.0, 20.0)
    vec.step(act)
    torch.cuda.synchronize()
    # `memory_allocated` counts the whole process: environments of earlier tests sit in reference cycles until Python's
    # collector runs, and one run in mid-loop freed their blocks between two readings.  So they are collected first, and the
    # collector stays off while the steps are counted -- cyclic garbage of a step itself would then show as growth.
    gc.collect()
    gc.disable()
    allocated = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            out = vec.step(act)
            allocated.append(torch.cuda.memory_allocated())
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    assert allocated[1] == allocated[4] and allocated[1:] == [allocated[1]] * 4, allocated
    assert out[0].shape == (4096, 28) and bool(torch.isfinite(out[0]).all()) and float(vec.normalizer.count[0]) > 4096 * 6
