"""Snapshot, restore and fork on the MI355X (sparc_amd/snapshot.py, sparc_amd/csrc/wedm_copy.h):
`wedm_copy_columns` against the plain-torch path bit for bit on raw planes of random bytes, its memory contract inside
guard bands, its bounds check, and the environment's three methods against the CPU oracle twin, which runs the torch path.

Shapes.  The kernel takes another path per element width (1, 4, 8, 16 bytes), per item size (rows 1, 7: one partial item;
8: one full item; 9, 33: full items and a partial one) and per position of a pair in its block of 256 (counts 1, 63, 64, 65,
255, 256, 257: a lane, a wave and a block, each one short, exact and one over).  257 distinct destinations need planes of
more than 257 columns, so the counts run on 300 columns at strides 320 (source) and 384 (destination); the strides 64
against 128, and 75 (no multiple of anything), run the counts their columns can hold."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from sparc_amd import _abi
from sparc_amd.snapshot import STATUS_OVERLAP, STATUS_RANGE, torch_copy_columns
from tests._snapshot_common import WINDOW, assert_same, everything, make, scenario

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5                       # as tests/_arena.py fills its arenas
ROWS = (1, 7, 8, 9, 33)
COUNTS = (1, 63, 64, 65, 255, 256, 257)
# (source stride, source columns, destination stride, destination columns)
SHAPES = ((320, 300, 384, 300), (64, 64, 128, 70), (128, 100, 75, 75), (75, 70, 75, 64))
DTYPES = {1: torch.uint8, 4: torch.int32, 8: torch.int64, 16: torch.float32}


class Plane:
    """A ``[rows][stride]`` block of elements of ``width`` bytes inside a guard arena: random bytes in the block, padding
    columns included (NaN payloads of every kind among them), ``FILL`` in the bands before and after it."""

    def __init__(self, gen, rows, stride, width, band=4096):
        self.rows, self.stride, self.width, self.band = rows, stride, width, band
        n = rows * stride * width
        self.raw = torch.full((2 * band + n,), FILL, dtype=torch.uint8, device=DEV)
        self.raw[band: band + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=gen)
        body = self.raw[band: band + n].view(DTYPES[width])
        self.tensor = body.view(rows, stride, 4) if width == 16 else body.view(rows, stride)   # what the torch path takes
        assert self.tensor.data_ptr() % 16 == 0

    def bytes(self) -> np.ndarray:
        return self.raw.cpu().numpy().copy()

    def expected(self, before: np.ndarray, src_bytes: np.ndarray, src_plane: "Plane", pairs) -> np.ndarray:
        """The arena after the copy, formed on the raw bytes: the named columns of the rows, and nothing else."""
        want = before.copy()
        d = want[self.band: self.band + self.rows * self.stride * self.width].reshape(self.rows, self.stride, self.width)
        s = src_bytes[src_plane.band: src_plane.band + src_plane.rows * src_plane.stride * src_plane.width]
        s = s.reshape(src_plane.rows, src_plane.stride, src_plane.width)
        for a, b in pairs:
            d[:, b] = s[:, a]
        return want


def _cplane(src: Plane, dst: Plane, src_cols, dst_cols):
    return _abi.CopyPlane(src.tensor.data_ptr(), dst.tensor.data_ptr(), src.rows, src.width, src.stride, dst.stride, src_cols, dst_cols)


def _backend():
    """The call itself is stateless; a backend object carries the stream and device handling."""
    env = make(DEV, 4)
    return env, env._backend


def _index_lists(rng, count, src_cols, dst_cols):
    """contiguous, reversed, strided, one source broadcast, a random permutation -- destinations always distinct."""
    base = np.arange(count)
    step = next(k for k in (7, 11, 13, 3) if np.gcd(k, dst_cols) == 1)
    yield "contiguous", (base + (src_cols - count)) % src_cols, base + (dst_cols - count)
    yield "reversed", base % src_cols, (dst_cols - 1 - base)
    yield "strided", (base * 3) % src_cols, (base * step) % dst_cols
    yield "broadcast", np.full(count, src_cols - 1), base
    yield "permutation", rng.permutation(src_cols)[:count] if count <= src_cols else rng.integers(0, src_cols, count), \
        rng.permutation(dst_cols)[:count]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)


@pytest.mark.parametrize("width", [1, 4, 8, 16])
def test_kernel_equals_the_torch_path_bit_for_bit(width):
    """Five planes per call (every row count), every shape, count and index list: the destination planes equal what
    ``index_select`` / ``index_copy_`` make of the same inputs, in every byte of the block (padding columns included), and
    the sources keep every byte."""
    env, be = _backend()
    gen = torch.Generator(device=DEV).manual_seed(width)
    rng = np.random.default_rng(width)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    calls = 0
    for ss, sc, ds, dc in SHAPES:
        srcs = [Plane(gen, r, ss, width) for r in ROWS]
        dsts = [Plane(gen, r, ds, width) for r in ROWS]
        src_before = [p.raw.clone() for p in srcs]
        for count in (c for c in COUNTS if c <= dc):
            for name, s, d in _index_lists(rng, count, sc, dc):
                assert len(set(d.tolist())) == count and d.min() >= 0 and d.max() < dc and s.min() >= 0 and s.max() < sc
                want = [p.tensor.clone() for p in dsts]
                torch_copy_columns([(a.tensor, w) for a, w in zip(srcs, want)], _dev(s).long(), _dev(d).long())
                si, di = _dev(s), _dev(d)
                be.copy_columns([_cplane(a, b, sc, dc) for a, b in zip(srcs, dsts)], si.data_ptr(), di.data_ptr(), count,
                                status.data_ptr())
                for r, b, w in zip(ROWS, dsts, want):
                    assert torch.equal(b.tensor.view(torch.uint8), w.view(torch.uint8)), (width, (ss, sc, ds, dc), count, name, r)
                calls += 1
        for p, before in zip(srcs, src_before):
            assert torch.equal(p.raw, before)
        for p in dsts:
            assert bool((p.raw[: p.band] == FILL).all()) and bool((p.raw[-p.band:] == FILL).all())
    assert int(status.item()) == 0 and calls == 5 * (7 + 4 + 4 + 3)
    env.close()


def test_sixteen_planes_of_every_width_in_one_call_inside_guard_bands():
    """The memory contract: after the copy the bytes that differ are exactly the destination columns of the named rows --
    padding columns, both bands and every source byte are untouched.  16 planes: every width with every partial and full
    item size."""
    env, be = _backend()
    gen = torch.Generator(device=DEV).manual_seed(16)
    rng = np.random.default_rng(16)
    shapes = [(w, r) for w in (1, 4, 8, 16) for r in (1, 7, 8, 33)]
    srcs = [Plane(gen, r, 128, w) for w, r in shapes]
    dsts = [Plane(gen, r, 75, w) for w, r in shapes]
    sc, dc, count = 100, 70, 65
    s, d = rng.integers(0, sc, count), rng.permutation(dc)[:count]
    src_before, dst_before = [p.bytes() for p in srcs], [p.bytes() for p in dsts]
    si, di = _dev(s), _dev(d)   # (held: a temporary's memory is handed to the next allocation at once)
    be.copy_columns([_cplane(a, b, sc, dc) for a, b in zip(srcs, dsts)], si.data_ptr(), di.data_ptr(), count, None)
    torch.cuda.synchronize()
    for a, b, sb, db in zip(srcs, dsts, src_before, dst_before):
        assert np.array_equal(a.bytes(), sb), "a source byte changed"
        got, want = b.bytes(), b.expected(db, sb, a, zip(s.tolist(), d.tolist()))
        assert np.array_equal(got, want), (b.width, b.rows, np.flatnonzero(got != want)[:8])
        assert (got != db).any()
    with pytest.raises(Exception, match="WEDM_ERR_BAD_ARG"):
        be.copy_columns([_cplane(srcs[0], dsts[0], sc, dc)] * 17, si.data_ptr(), di.data_ptr(), count, None)
    env.close()


def test_indices_out_of_range_copy_nothing_and_set_the_status_word():
    """The bounds check is the kernel's own: the index lists are device data nobody has read.  Pairs with a source or a
    destination outside the plane's columns -- negative, the first padding column, the stride, far outside -- are skipped,
    the valid pairs are copied, nothing outside the named columns changes, bit 0 of the status word is set; in-place too."""
    env, be = _backend()
    gen = torch.Generator(device=DEV).manual_seed(5)
    for width in (1, 4, 8, 16):
        a, b = Plane(gen, 9, 128, width), Plane(gen, 9, 75, width)
        sc, dc = 100, 70
        s = np.array([0, -1, 5, sc, 7, 128, 9, 2**31 - 1, 11, 3, -2**31, 99])
        d = np.array([1, 2, -1, 3, dc, 4, 75, 5, 2**31 - 1, 69, 6, 0])
        ok = [(x, y) for x, y in zip(s.tolist(), d.tolist()) if 0 <= x < sc and 0 <= y < dc]
        assert len(ok) == 3
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        sb, db = a.bytes(), b.bytes()
        si, di = _dev(s), _dev(d)
        be.copy_columns([_cplane(a, b, sc, dc)], si.data_ptr(), di.data_ptr(), len(s), status.data_ptr())
        be.copy_columns([_cplane(a, b, sc, dc)], si.data_ptr(), di.data_ptr(), len(s), None)   # no word: skipped silently
        torch.cuda.synchronize()
        assert int(status.item()) == STATUS_RANGE
        assert np.array_equal(a.bytes(), sb) and np.array_equal(b.bytes(), b.expected(db, sb, a, ok)), width
        # in place (a fork): valid pairs 0 -> 60 and 1 -> 61, the others outside [0, 64)
        s, d = np.array([0, 64, 1, 2]), np.array([60, 3, 61, 64])
        status.zero_()
        sb = a.bytes()
        si, di = _dev(s), _dev(d)
        be.copy_columns([_cplane(a, a, 64, 64)], si.data_ptr(), di.data_ptr(), 4, status.data_ptr())
        torch.cuda.synchronize()
        assert int(status.item()) == STATUS_RANGE and np.array_equal(a.bytes(), a.expected(sb, sb, a, [(0, 60), (1, 61)]))
    env.close()


# ------------------------------------------------------------------------------------------------ the environment
N = 70


def _pair(binding, geometry):
    gpu, cpu = make(DEV, N, binding, geometry), make("cpu", N, binding, geometry)
    return gpu, cpu, scenario(gpu), scenario(cpu)


def _agree(gpu, cpu, where):
    torch.cuda.synchronize()
    assert_same(everything(gpu), everything(cpu), where)   # every byte of every block and bound row, padding included


@pytest.mark.parametrize("geometry", ["s128", "s13"])
@pytest.mark.parametrize("binding", ["plain", "all"])
def test_environment_against_the_cpu_twin_after_every_operation(binding, geometry):
    """70 environments at stride 128, sparking and terminating in mid-interval: snapshot, 400 us, restore of a subset
    (permuted columns, one into another slot), fork of 3 sources into 40 destinations, 400 us -- the same calls on both
    sides, the twin on the torch path.  ``plain`` runs the automatic kernel choice, ``all`` pulse and signal statistics,
    per-environment parameters and materials and a crater log together."""
    gpu, cpu, act_g, act_c = _pair(binding, geometry)
    assert gpu.state.stride == 128 and gpu.n_segments == (128 if geometry == "s128" else 13)
    for env, act in ((gpu, act_g), (cpu, act_c)):
        env.step_many(act, 150)
    _agree(gpu, cpu, "before")
    ids = [3, 68, 69, 0, 17, 35, 36]
    snap_g, snap_c = gpu.snapshot(torch.tensor(ids, device=DEV)), cpu.snapshot(ids)
    torch.cuda.synchronize()
    assert snap_g.stride == 64 and snap_g.device.type == "cuda"
    assert_same({k: v.cpu() for k, v in snap_g.blocks.items()}, snap_c.blocks, "the snapshots")
    for env, act in ((gpu, act_g), (cpu, act_c)):
        env.step_many(act, 400)
    name = gpu._backend.last_kernel()
    if binding == "all":
        assert "wedm_step_global" in name and all(tag in name for tag in ("[pulse]", "[envp]", "[wmat]", "[sig]")), name
    elif geometry == "s128":
        assert "wedm_step_regs" in name, name   # the automatic choice for a small batch: the wide register kernel
    _agree(gpu, cpu, "stepped")
    gpu.restore(snap_g, env_ids=torch.tensor([69, 3, 0, 20], device=DEV), columns=torch.tensor([2, 0, 3, 4], device=DEV))
    cpu.restore(snap_c, env_ids=[69, 3, 0, 20], columns=[2, 0, 3, 4])
    _agree(gpu, cpu, "restored")
    src = np.repeat([3, 69, 20], [14, 13, 13])
    dst = np.array([e for e in range(N) if e not in (3, 69, 20)])[:40]
    gpu.fork(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV))
    cpu.fork(src, dst)
    _agree(gpu, cpu, "forked")
    got = everything(gpu)
    assert_same(got, got, "destinations equal their sources", cols_got=dst.tolist(), cols_want=src.tolist())
    for env, act in ((gpu, act_g), (cpu, act_c)):
        env.step_many(act, 400)
    _agree(gpu, cpu, "stepped on")
    gpu.check_errors()
    assert int(gpu.state.spark_count.sum()) > 100 and bool(gpu.state.done.any())
    gpu.close()


@pytest.mark.parametrize("binding", ["plain", "all"])
def test_replay_on_the_device(binding):
    """tests/test_snapshot_host.py's round trip and replay, through the kernel."""
    env = make(DEV, N, binding)
    act = scenario(env)
    env.step_many(act, 150)
    at_snapshot = everything(env)
    snap = env.snapshot()
    for k in WINDOW:
        env.step_many(act, k)
    first = everything(env)
    env.restore(snap)
    assert_same(everything(env), at_snapshot, "restored")
    for k in WINDOW:
        env.step_many(act, k)
    assert_same(everything(env), first, "replayed")
    assert int(env.state.spark_count.sum()) > 0
    env.close()


def test_device_indices_are_never_read_back_and_their_mistakes_reach_check_errors():
    env = make(DEV, 4096)
    act = scenario(env)
    env.step_many(act, 50)
    src = torch.arange(64, device=DEV)
    dst = torch.arange(64, 128, device=DEV)
    env.fork(src, dst)   # (first use: code object loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        env.fork(src, dst + 1000)
        env.fork(src[:1], dst + 2000)
        snap = env.snapshot(dst)
        env.restore(snap)
        env.restore(snap, env_ids=dst + 3000, columns=src)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    env.check_errors()
    bits = env.state.f64.view(torch.int64)   # (SPARK_Y is NaN: compared as bits)
    assert torch.equal(bits[:, 1000 + 64: 1000 + 128], bits[:, :64]) and torch.equal(bits[:, 3064: 3128], bits[:, 64: 128])
    for call, bit in ((lambda: env.fork(src, torch.cat([dst[:63], dst[:1]])), STATUS_OVERLAP),       # a destination twice
                      (lambda: env.fork(src, torch.cat([dst[:63], src[5:6]])), STATUS_OVERLAP),      # a source overwritten
                      (lambda: env.fork(src, torch.cat([dst[:63], dst[:1] + 4096])), STATUS_RANGE),
                      (lambda: env.restore(snap, env_ids=torch.cat([dst[:63], dst[:1]])), STATUS_OVERLAP),
                      (lambda: env.snapshot(dst - 65), STATUS_RANGE)):
        call()
        assert int(env._copy_status.item()) == bit
        with pytest.raises(ValueError, match="indices in a device tensor"):
            env.check_errors()
        env.check_errors()   # reported once
    env.close()
