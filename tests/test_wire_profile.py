"""The wire profile on the MI355X (sparc_amd/csrc/wedm_profile.h, sparc_amd/profile.py):
`wedm_wire_profile` against the definition written out in tests/_wire_profile_ref.py, bit for bit, on wire blocks whose
every dead cell is poisoned; its memory contract inside guard bands; its device-side checks; and the environment's and the
vector adapter's methods against the CPU oracle twin, which runs the host path.

Shapes.  The kernel cuts a wire's quads over the 4, 8 or 16 waves of a block (the host picks, for batches this small: 4 up
to 31 quads, 8 from 32, 16 from 64) and takes four quads per batch of loads, so the segment counts are: 1, 3, 4, 5 (one quad
and two: waves without a cell), 13 (a tail quad with one cell), 127 / 128 / 130 (32 quads on 8 waves, one cell short and
exact, and 33: chunks of 5, a short seventh wave and an empty eighth), 401 (101 quads on 16 waves: chunks of 7, the last
wave empty), 1201 (301 quads on 16 waves: chunks of 19, five batches of loads each).  Batches: 1, 5 (one partial
wave), 64 (exactly one), 70, 257 (several blocks and a partial one).  Bins: 0 (none), 1, 3 (uneven), 8, 16, 64 (more bins
than cells for the short wires: replication)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from sparc_amd import WireEDMVectorEnv, _abi
from sparc_amd.profile import STATUS_GEOMETRY, STATUS_RANGE
from tests._arena import FILL, Arena
from tests._snapshot_common import WINDOW, make, scenario
from tests._wire_profile_ref import bin_edges, pack, reference_rows, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BINS = (0, 1, 3, 8, 16, 64)
# (num_envs, n_seg_max, stride of T and the geometry rows, out_stride): every batch and every segment count of the docstring;
# strides that are multiples of 64 and that are not, out strides equal to and different from the stride
SHAPES = ((1, 1, 64, 64), (5, 3, 7, 5), (64, 4, 64, 128), (70, 5, 75, 70), (257, 13, 300, 320), (5, 127, 64, 75),
          (70, 128, 128, 128), (64, 130, 70, 64), (257, 401, 260, 257), (5, 1201, 64, 8), (70, 1201, 75, 128))
SENTINEL = np.float32(-7.25)   # what an output column holds before a launch


@pytest.fixture(scope="module")
def backend():
    """The call is stateless; a backend object carries the stream and device handling."""
    env = make(DEV, 4)
    yield env._backend
    env.close()


def _geometry(rng, num_envs, n_max, per_env):
    """Per-environment: wires of every length in [1, n_max] (the shortest and the longest among them) and zones of every
    kind (inside, reversed, past the end, negative, the whole wire).  Uniform: the longest wire, a zone inside it."""
    if not per_env:
        a, b = sorted(rng.integers(0, n_max + 1, 2))
        return np.full(num_envs, n_max), np.full(num_envs, a), np.full(num_envs, max(b, min(a + 1, n_max)))
    n = rng.integers(1, n_max + 1, num_envs)
    n[0], n[-1] = n_max, 1
    zs, ze = np.zeros(num_envs, dtype=np.int64), np.zeros(num_envs, dtype=np.int64)
    for e in range(num_envs):
        a, b = sorted(rng.integers(0, n[e] + 1, 2))
        zs[e], ze[e] = ((a, b), (b, a), (a, n[e] + 1 + e % 3), (-1, b), (0, n[e]))[e % 5]
    return n, zs, ze


def _geom_rows(n, zs, ze, stride, pad_n):
    """int32 [GEOM_I32_COUNT][stride]; the padding columns hold a wire length that must never be used."""
    g = np.full((_abi.GEOM_I32_COUNT, stride), -12345, dtype=np.int32)
    g[_abi.GI32.N_SEG, :] = pad_n
    g[_abi.GI32.N_SEG, : n.size], g[_abi.GI32.AZ_START, : n.size], g[_abi.GI32.AZ_END, : n.size] = n, zs, ze
    return torch.from_numpy(g).to(DEV)


class Call:
    """One wire block with its geometry on the device, and the launches on it."""

    def __init__(self, backend, cells, n, zs, ze, stride, per_env, dead, out_stride):
        self.be, self.num_envs, self.n_max = backend, cells.shape[0], cells.shape[1]
        self.per_env, self.stride, self.out_stride = per_env, stride, out_stride
        self.n, self.zs, self.ze = n, zs, ze
        self.T = torch.from_numpy(pack(cells, n, stride, dead)).to(DEV)
        assert self.T.data_ptr() % 16 == 0
        self.geom = _geom_rows(n, zs, ze, stride, pad_n=10 ** 6) if per_env else None
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def desc(self, bins, out, out_cols):
        u = not self.per_env
        return _abi.ProfileDesc(T=self.T.data_ptr(), stride=self.stride, num_envs=self.num_envs, n_seg_max=self.n_max,
                                n_seg=int(self.n[0]) if u else -1, az_start=int(self.zs[0]) if u else -1,
                                az_end=int(self.ze[0]) if u else -1, geom_i32=None if u else self.geom.data_ptr(),
                                bins=bins, out=out.data_ptr(), out_stride=self.out_stride, out_cols=out_cols)

    def run(self, bins, ids=None, out=None, out_cols=None, sync=True):
        """The ``[rows][out_stride]`` block after the launch (a fresh one full of SENTINEL unless given).  ``sync=False``
        only enqueues the launch on torch's current stream (tests/test_streams.py); the caller synchronises."""
        count = self.num_envs if ids is None else len(ids)
        if out is None:
            out = torch.full((_abi.profile_rows(bins), self.out_stride), float(SENTINEL), dtype=torch.float32, device=DEV)
        idx = None if ids is None else torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(DEV)
        self.be.wire_profile(self.desc(bins, out, count if out_cols is None else out_cols),
                             None if idx is None else idx.data_ptr(), count, self.status.data_ptr())
        if sync:
            torch.cuda.synchronize()
        return out


@pytest.mark.parametrize("per_env", [False, True], ids=["uniform", "per-env"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_definition_bit_for_bit_on_poisoned_blocks(backend, shape, per_env):
    """Every bin count; environment lists NULL, permuted, and repeated; and every cell of ``T`` that is not a live cell --
    from an environment's own n_seg up to n_seg_max, the tail quad, the columns from num_envs on -- holding 1e30, then NaN:
    the rows equal the definition computed from the live cells alone, and the columns from ``count`` on keep the sentinel."""
    num_envs, n_max, stride, out_stride = shape
    rng = np.random.default_rng(list(shape) + [int(per_env)])
    cells = rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32)
    n, zs, ze = _geometry(rng, num_envs, n_max, per_env)
    for e in range(0, num_envs, 3):   # tied maxima
        cells[e, rng.choice(n[e], size=min(3, n[e]), replace=False)] = np.float32(4000.5)
    want = {bins: reference_rows(cells, n, zs, ze, bins) for bins in BINS}
    lists = [None, rng.permutation(num_envs)[:out_stride], rng.integers(0, num_envs, min(out_stride, num_envs + 3))]
    for dead in (np.float32(1.0e30), np.float32(np.nan)):
        call = Call(backend, cells, n, zs, ze, stride, per_env, dead, out_stride)
        T_before = call.T.clone()
        for bins in BINS:
            for ids in lists:
                if ids is None and num_envs > out_stride:
                    continue
                got = call.run(bins, ids).cpu().numpy()
                count = num_envs if ids is None else len(ids)
                ref = want[bins] if ids is None else want[bins][:, ids]
                assert same_bits(got[:, :count], ref), (shape, per_env, str(dead), bins, None if ids is None else "list",
                                                        np.argwhere(got[:, :count] != ref)[:5].tolist())
                assert (got[:, count:] == SENTINEL).all()
        assert int(call.status.item()) == 0
        assert torch.equal(call.T.view(torch.int32), T_before.view(torch.int32))


@pytest.mark.parametrize("per_env", [False, True], ids=["uniform", "per-env"])
@pytest.mark.parametrize("n_max", [13, 130, 401, 1201])
def test_a_maximum_planted_in_every_cell_is_found_where_it_is(backend, n_max, per_env):
    """One environment per cell of the wire: environment e has its maximum at cell e (so in the first cell, the last, on
    both sides of every quad boundary, of every bin boundary and of every boundary between two waves' runs of quads), and
    the same value again at a later cell in every second environment.  NaN in every dead cell."""
    rng = np.random.default_rng(n_max)
    num_envs = n_max
    cells = rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32)
    n = np.full(num_envs, n_max) if not per_env else np.maximum(np.arange(num_envs) + 1, n_max - np.arange(num_envs) % 7)
    spot = np.arange(num_envs)   # < n[e] in both cases
    later = np.minimum(spot + 1 + rng.integers(0, 9, num_envs), n - 1)
    cells[spot, spot] = np.float32(5000.25)
    cells[spot[::2], later[::2]] = np.float32(5000.25)
    zs, ze = np.full(num_envs, n_max // 3), np.full(num_envs, n_max // 3 + max(1, n_max // 4))
    stride = (num_envs + 63) // 64 * 64
    call = Call(backend, cells, n, zs, ze, stride, per_env, np.float32(np.nan), stride)
    for bins in (8, 3):
        got = call.run(bins).cpu().numpy()[:, :num_envs]
        assert same_bits(got, reference_rows(cells, n, zs, ze, bins)), (n_max, per_env, bins)
        assert (got[_abi.PR.HOT_CELL] == spot).all() and (got[_abi.PR.WIRE_MAX] == np.float32(5000.25)).all()
        for e in (0, n_max // 2, n_max - 1):
            b = next(k for k, (lo, hi) in enumerate(bin_edges(int(n[e]), bins)) if lo <= e < hi)
            assert got[_abi.PR_FIXED + b, e] == np.float32(5000.25)
    assert int(call.status.item()) == 0


def test_only_the_named_columns_of_out_change_inside_guard_bands(backend):
    """``out`` inside 0xA5 guard bands, more columns allowed than asked for: the bytes that differ after a launch lie in rows
    x columns [0, count); ``T`` and the geometry rows keep every byte."""
    rng = np.random.default_rng(5)
    num_envs, n_max, stride, out_stride = 70, 130, 75, 100
    cells = rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32)
    for per_env in (False, True):
        n, zs, ze = _geometry(rng, num_envs, n_max, per_env)
        call = Call(backend, cells, n, zs, ze, stride, per_env, np.float32(1.0e30), out_stride)
        T_before = call.T.clone()
        geom_before = None if call.geom is None else call.geom.clone()
        for bins, ids in ((8, None), (64, None), (0, list(range(69, 30, -1))), (3, [4] * 90)):
            count = num_envs if ids is None else len(ids)
            arena = Arena("out", torch.empty((_abi.profile_rows(bins), out_stride), dtype=torch.float32, device=DEV),
                          out_stride, count)
            before = arena.raw.cpu().numpy().copy()
            call.run(bins, ids, out=arena.view, out_cols=min(out_stride, count + 7))
            after = arena.raw.cpu().numpy()
            stray = np.flatnonzero((before != after) & ~arena.owned_mask())
            assert stray.size == 0, (per_env, bins, [arena.locate(int(k)) for k in stray[:5]])
            ref = reference_rows(cells, n, zs, ze, bins, ids)
            assert same_bits(arena.view[:, :count].cpu().numpy(), ref)
            assert (arena.view[:, count:].contiguous().view(torch.uint8) == FILL).all()
        assert torch.equal(call.T.view(torch.int32), T_before.view(torch.int32))
        assert geom_before is None or torch.equal(call.geom, geom_before)
        assert int(call.status.item()) == 0


def test_bad_indices_and_geometry_rows_set_the_status_word_and_leave_their_columns(backend):
    rng = np.random.default_rng(6)
    num_envs, n_max, stride = 70, 13, 128
    cells = rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32)
    n, zs, ze = _geometry(rng, num_envs, n_max, True)
    good = reference_rows(cells, n, zs, ze, 8)
    # indices out of range, in a device list nobody has read
    for per_env in (False, True):
        nn, a, b = (n, zs, ze) if per_env else _geometry(rng, num_envs, n_max, False)
        ref = reference_rows(cells, nn, a, b, 8)
        call = Call(backend, cells, nn, a, b, stride, per_env, np.float32(np.nan), stride)
        ids = np.array([3, -1, 69, 70, 0, 2 ** 31 - 1, 5, -2 ** 31, 128, 68], dtype=np.int64)
        bad = (ids < 0) | (ids >= num_envs)
        got = call.run(8, ids.astype(np.int32)).cpu().numpy()
        assert int(call.status.item()) == STATUS_RANGE
        assert (got[:, : ids.size][:, bad] == SENTINEL).all() and (got[:, ids.size:] == SENTINEL).all()
        assert same_bits(got[:, : ids.size][:, ~bad], ref[:, ids[~bad]])
        call.status.zero_()
        call.be.wire_profile(call.desc(8, torch.empty((20, stride), device=DEV), ids.size),
                             torch.from_numpy(ids.astype(np.int32)).to(DEV).data_ptr(), ids.size, None)   # no status word
        torch.cuda.synchronize()
        assert int(call.status.item()) == 0
    # geometry rows with an n_seg outside [1, n_seg_max]
    call = Call(backend, cells, n, zs, ze, stride, True, np.float32(np.nan), stride)
    wrong = {7: 0, 8: n_max + 1, 40: -5, 69: 2 ** 31 - 1}
    for e, v in wrong.items():
        call.geom[_abi.GI32.N_SEG, e] = v
    got = call.run(8).cpu().numpy()
    assert int(call.status.item()) == STATUS_GEOMETRY
    ok = np.array([e not in wrong for e in range(num_envs)])
    assert (got[:, :num_envs][:, ~ok] == SENTINEL).all() and same_bits(got[:, :num_envs][:, ok], good[:, ok])
    call.status.zero_()
    got = call.run(8, [7, 200, 6]).cpu().numpy()
    assert int(call.status.item()) == (STATUS_RANGE | STATUS_GEOMETRY)
    assert (got[:, :2] == SENTINEL).all() and same_bits(got[:, 2], good[:, 6])
    spare = torch.empty((134, stride), device=DEV)
    with pytest.raises(Exception, match="wedm_wire_profile: bins"):
        call.be.wire_profile(call.desc(65, spare, 70), None, 70, None)


# ------------------------------------------------------------------------------------------------ the environment
N = 70


@pytest.mark.parametrize("binding,geometry,kernel", [("plain", "s128", 0), ("plain", "s13", 0), ("wmat", "s128", 2)])
def test_environment_profile_equals_the_cpu_twins(binding, geometry, kernel):
    """70 environments after the 300 us of the snapshot tests' scenario, on the automatic kernel choice and, with
    per-environment materials (per-environment geometry rows), on kernel 2: every row equals the CPU oracle twin's, which the
    host path computes; ``wire_max`` is ``state.wire_max_temperature``; with per-environment geometry
    `zone_mean_temperature` is the profile's row."""
    gpu, cpu = make(DEV, N, binding, geometry), make("cpu", N, binding, geometry)
    if kernel:
        gpu.set_kernel(kernel)
    for env in (gpu, cpu):
        act = scenario(env)
        for k in WINDOW:
            env.step_many(act, k)
    if binding == "wmat":
        assert gpu.geometry is None and "[wmat]" in gpu._backend.last_kernel(), gpu._backend.last_kernel()
    for bins, ids in ((8, None), (64, None), (3, [69, 0, 0, 35])):
        got = gpu.wire_profile(bins, ids if ids is None else torch.tensor(ids, device=DEV))
        want = cpu.wire_profile(bins, ids)
        assert got["rows"].shape == want["rows"].shape and got["rows"].device.type == "cuda"
        assert same_bits(got["rows"].cpu().numpy(), want["rows"].numpy()), (binding, geometry, bins)
        assert same_bits(got["bin_mean"].cpu().numpy(), want["bin_mean"].numpy())
    assert same_bits(gpu.wire_profile()["wire_max"].cpu().numpy(), gpu.state.wire_max_temperature.to(torch.float32).cpu().numpy())
    if gpu.geometry is None:   # (uniform geometry keeps its float32 torch mean, whose order differs between the devices)
        assert same_bits(gpu.zone_mean_temperature().cpu().numpy(), cpu.zone_mean_temperature().numpy())
        assert same_bits(gpu.zone_mean_temperature().cpu().numpy(), cpu.wire_profile(0)["zone_mean"].numpy())
    assert len(set(cpu.wire_profile()["wire_max"].tolist())) > 10
    gpu.check_errors()
    gpu.close()


def test_vector_env_steps_without_a_synchronisation_and_device_indices_reach_check_errors():
    env = make(DEV, 4096, "autoreset")
    vec = WireEDMVectorEnv(env, wire_profile_bins=8)
    obs, _ = vec.reset(seed=3)
    d = env.obs_dim
    assert obs.shape == (4096, d + 20) and len(vec.obs_names) == d + 20
    env.state.workpiece_position = torch.linspace(10.4, 25.0, 4096, dtype=torch.float64, device=DEV)
    env.state.wire_position = 10.0
    action = env.make_action(0.0, 80.0, 9, 3.0, 30.0)
    ids = torch.tensor([5, 4095, 5, 0], device=DEV)
    vec.step(action)                # (first use: code objects loaded)
    env.wire_profile(3, ids)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            obs = vec.step(action)[0]
        some = env.wire_profile(3, ids)["rows"].clone()
        env.wire_profile(3, ids + 1)    # one index out of range: skipped on the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert obs.shape == (4096, d + 20)
    assert same_bits(obs[:, d:].t().cpu().numpy(), env.wire_profile(8)["rows"].cpu().numpy())
    assert same_bits(obs[:, d + _abi.PR.WIRE_MAX].cpu().numpy(), env.state.wire_max_temperature.to(torch.float32).cpu().numpy())
    assert same_bits(some.cpu().numpy(), env.wire_profile(3)["rows"][:, [5, 4095, 5, 0]].cpu().numpy())
    assert len(set(obs[:, d + _abi.PR.WIRE_MAX].tolist())) > 10
    assert int(env._profile_status.item()) == STATUS_RANGE
    with pytest.raises(ValueError, match="wire_profile with indices in a device tensor"):
        env.check_errors()
    env.check_errors()   # reported once
    env.close()
