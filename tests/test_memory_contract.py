"""The memory contract of the C-ABI (include/wedm_hip.h, "What a launch writes"): `wedm_step` and
`wedm_reset` write columns ``[0, num_envs)`` of the rows of the bound state blocks (and of the pulse block, and the slots
of a bound trace ring) and nothing else -- not the padding columns ``[num_envs, stride)``, not a byte before a block's
first row or after its last one, not the action leaves, the reset mask, the geometry / env-param / wire-material rows or
the replay table -- at every ``stride >= num_envs``, with the same results in the owned columns.

Every block lives in a guard arena (tests/_arena.py): bands of at least two rows and 4 KB on both sides, everything
pre-filled with 0xA5.  After every launch the arenas are compared byte by byte outside the ownership mask FIRST, then the
owned columns with the CPU oracle, bit for bit.  The CPU part checks the harness itself on the oracle (which keeps the
contract) and that the checker names a poked byte's block and region.

Shapes are the smallest at which a guard can be missing, not the workload's: 1 (one live lane), 5 (a partial wave at 16
lanes per environment), 25 / 49 (one environment past a served block of 24 / 48), 65 (one live environment in the second
wave, 63 padding columns), 100 (a ragged last block of 128); wires of 128 segments (the register kernels' limit), 400
(default) and 129 (three padding cells in the last word of T).

Not covered: the device copy of `wedm_params` (the library owns it; nothing on this side of the ABI can read it).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from sparc_amd import WireEDMEnv, WireModuleParameters
from tests._arena import REGIONS, action_leaves, assert_inputs_unchanged, clone_inputs, guarded
from tests._compare import block_diffs
from tests._oracle_backend import OracleBackend, OracleBackendRows
from tests.test_gpu_parity import KERNELS, SERVED, SERVED_ANY

LAUNCHES = (1, 7, 1100)   # a single microsecond, a short fused launch, one that crosses a control step
ACTION = (0.05, 80.0, 13, 2.0, 20.0)
SEED = 11
WIRES = {128: dict(wire_params=WireModuleParameters(segment_len=0.625)), 400: {},
         129: dict(wire_params=WireModuleParameters(segment_len=80.0 / 129.5))}
BASE = dict(autoreset=True, reward="progress", crater_log_capacity=8)
FAMILY = {1: "wedm_step_global", 2: "wedm_step_lanes_pk<", 3: "wedm_step_fused<", 4: "wedm_step_packed<", 5: "wedm_step_split",
          6: "wedm_step_stream<", 7: "wedm_step_regs<", 8: "wedm_step_regs_wide<", 9: "wedm_step_served<", 10: "wedm_step_lanes<",
          11: "wedm_step_lanes_served<", 12: "wedm_step_regs_served<"}


def form_kw(form, n):
    """Constructor keywords of a form (every optional writer of the ABI once) and whether the oracle needs its rows seam."""
    if form == "base":
        return dict(BASE), False
    if form == "pulse":
        return dict(BASE, pulse_stats=True), True
    if form == "f64":
        return dict(BASE, stencil_dtype="float64"), False
    if form == "trace":   # (the oracle's seam samples between sub-launches: no per-launch reward, no in-launch reset with it)
        return dict(crater_log_capacity=8), False
    if form == "keep":    # terminated environments keep being stepped (no freeze, no in-launch reset)
        return dict(reward="progress", crater_log_capacity=8, freeze_terminated=False), False
    geom = dict(workpiece_height=np.linspace(10.0, 30.0, n), wire_diameter=np.resize([0.1, 0.2, 0.3], n))
    if form == "geom":
        return dict(BASE, **geom), False
    if form == "rows":    # per-environment physics rows and wire material on per-environment geometry
        from tests._envp_draw import omega_26bit
        from tests._wmat_draw import BRASS, COPPER

        rng = np.random.default_rng(5)
        envp = {"plasma_efficiency": rng.uniform(0.05, 0.3, n), "base_critical_density": rng.uniform(0.05, 0.4, n),
                "omega_n": omega_26bit(rng.uniform(150.0, 400.0, n))}
        return dict(BASE, env_params=envp, wire_material=[(BRASS, COPPER)[e % 2] for e in range(n)], **geom), True
    raise KeyError(form)


def make_env(n, segs, form, device):
    kw, rows = form_kw(form, n)
    backend = {} if device != "cpu" else dict(backend=OracleBackendRows if rows else OracleBackend)
    env = WireEDMEnv(num_envs=n, device=device, **backend, **WIRES[segs], **kw)
    assert form in ("geom", "rows") or env.n_segments == segs
    return env


def scenario(env):
    """A narrow gap for dense sparking; every fifth environment's target lies just behind its first crater (it terminates
    inside the long launch) and every fifth one's is already reached (it terminates in the first microsecond, so the
    second launch resets it inside the kernel, or finds it frozen)."""
    n = env.num_envs
    e = torch.arange(n)
    env.reset(seed=SEED)
    env.state.workpiece_position = 14.0
    env.state.wire_position = 10.0
    env.state.target_position = torch.where(e % 5 == 0, 14.0005, torch.where(e % 5 == 2, 13.0, 5000.0)).to(torch.float64)


def extra_diffs(got, want, n):
    """The blocks `block_diffs` leaves out: the crater ring (the slots written so far) and the pulse rows."""
    out = []
    G, W = got.state, want.state
    if G.crater_log is not None:
        g, w = G.crater_log[:, :n].cpu(), W.crater_log[:, :n].cpu()
        filled = torch.arange(g.shape[0])[:, None] < G.spark_count.cpu()[None, :]
        if not torch.equal(torch.where(filled, g, 0), torch.where(filled, w, 0)):
            out.append("crater_log differs")
    if G.pulse is not None and not torch.equal(G.pulse[:, :n].cpu(), W.pulse[:, :n].cpu()):
        out.append("pulse rows differ")
    return out


def owned_bytes(env):
    n = env.num_envs
    return {k: v[:, :n].contiguous().numpy().tobytes() for k, v in env.state.clone_blocks().items()}


def run_case(env, twin, guard, variant=0, lanes=0, launches=LAUNCHES, expect=None, after_launch=None):
    """The steps every case takes: scenario, snapshot, the launches and a masked and a full reset, each followed by the
    byte comparison outside the ownership mask and then the bit-exact comparison of the owned columns with `twin` (an
    environment stepped alongside: the oracle, or None).  Returns {launch: kernel string} of the launches that ran and
    the owned columns after each step (launches refused as WEDM_ERR_UNSUPPORTED are skipped on both sides)."""
    from sparc_amd._lib import WedmError

    n = env.num_envs
    envs = [env] + ([twin] if twin is not None else [])
    acts = [e.make_action(*ACTION) for e in envs]
    names, leaves = action_leaves(acts[0])
    ran, stages = {}, []

    def check(what, before):
        after = guard.snapshot()
        guard.assert_only_owned_changed(before, after)
        if twin is not None:
            diffs = block_diffs(env.state.clone_blocks(), twin.state.clone_blocks(), n) + extra_diffs(env, twin, n)
            assert not diffs, f"{what}: kernel {env._backend.last_kernel()} (n={n}, S={env.n_segments}, stride={env.state.stride}):\n" + \
                "\n".join(diffs[:12])
        stages.append(owned_bytes(env))
        return after

    before = guard.snapshot()
    for k in launches:
        held = clone_inputs(*leaves)
        try:
            env.step_many(acts[0], k)
        except WedmError as exc:
            assert "UNSUPPORTED" in str(exc)
            continue
        if twin is not None:
            twin.step_many(acts[1], k)
        before = check(f"after {k} us", before)
        kernel = ran[k] = env._backend.last_kernel()
        assert_inputs_unchanged(names, leaves, held, kernel)
        if expect is not None:   # a forced kernel that fell back to another family would pass the comparison unnoticed
            want = expect(k) if callable(expect) else expect
            assert kernel.startswith(want), f"forced kernel {variant} lanes {lanes}, launch of {k} us ran {kernel}"
        if after_launch is not None:
            after_launch(k)
    for mask, seed in ((np.arange(n) % 3 == 1, None), (None, SEED + 1)):
        for e in envs:
            e.reset(seed=seed, options=None if mask is None else {"mask": mask})
        before = check("after the masked reset" if mask is not None else "after the full reset", before)
        if mask is not None:
            assert torch.equal(env._mask_buf.cpu(), torch.as_tensor(mask).to(torch.uint8)), "the reset mask was written"
    return ran, stages


# ------------------------------------------------------------------------------------------------------ CPU part
def test_oracle_keeps_the_contract_in_guard_arenas_and_equals_an_unguarded_twin():
    n = 65
    env, twin = make_env(n, 400, "base", "cpu"), make_env(n, 400, "base", "cpu")
    scenario(env), scenario(twin)
    guard = guarded(env)
    assert set(guard.arenas) == {"f64", "i32", "i8", "T", "obs", "stats", "reward", "crater_log"}
    for name, a in guard.arenas.items():   # bands: two rows of the block and 4 KB at least, filled with the pattern
        band = a.lead * a.itemsize
        assert band >= 4096 and a.lead >= 2 * a.width * a.inner, name
        raw = a.raw.numpy()
        assert (raw[:band] == 0xA5).all() and (raw[-band:] == 0xA5).all(), name
    changed = set()
    first = guard.snapshot()

    def note(k):
        now = guard.snapshot()
        changed.update(name for name in now if (now[name] != first[name]).any())

    ran, _ = run_case(env, twin, guard, after_launch=note)
    assert sorted(ran) == [1, 7, 1100]
    assert changed == set(guard.arenas)                      # the owned columns did change, in every block
    assert int(twin.state.spark_count.max()) == 0            # (after the full reset)


def test_oracle_optional_blocks_keep_the_contract_in_guard_arenas():
    """The pulse block, and the geometry, env-param and wire-material rows (never written) on the oracle's rows seam."""
    n = 65
    for form, segs, names in (("pulse", 128, {"pulse"}), ("rows", 128, {"_geom_f64", "_geom_i32", "_envp_rows", "_wmat_rows"})):
        env, twin = make_env(n, segs, form, "cpu"), make_env(n, segs, form, "cpu")
        scenario(env), scenario(twin)
        guard = guarded(env)
        assert names <= set(guard.arenas)
        ran, _ = run_case(env, twin, guard)
        assert sorted(ran) == [1, 7, 1100]


def test_oracle_trace_rings_in_guard_arenas():
    n = 65
    env, twin = make_env(n, 128, "trace", "cpu"), make_env(n, 128, "trace", "cpu")
    scenario(env), scenario(twin)
    guard = guarded(env)
    tr, tt = (e.bind_trace(["voltage", "time", "spark_state"], every=3, capacity=5, envs=(7, 9), wire_temperature=True)
              for e in (env, twin))
    guard.guard_trace(tr)
    assert {"trace.f64", "trace.i32", "trace.i8", "trace.T"} <= set(guard.arenas)
    run_case(env, twin, guard)
    assert tr.count == tt.count == 1108 // 3 and tr.count > tr.capacity
    a, b = tr.read(), tt.read()
    assert all(torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("region", REGIONS[:3])
def test_checker_names_the_block_and_the_region_of_a_poked_byte(region):
    n = 65
    env = make_env(n, 128, "pulse", "cpu")
    scenario(env)
    guard = guarded(env)
    assert set(guard.arenas) == {"f64", "i32", "i8", "T", "obs", "stats", "reward", "crater_log", "pulse"}
    for name, a in guard.arenas.items():
        row = a.width * a.inner
        at = {"before-band": a.lead - 1, "padding column": a.lead + (a.rows - 1) * row + n * a.inner,
              "after-band": a.lead + a.count}[region] * a.itemsize
        before = guard.snapshot()
        assert guard.violations(before, guard.snapshot()) == []
        a.raw[at] ^= 0xFF
        bad = guard.violations(before, guard.snapshot())
        assert len(bad) == 1 and bad[0].startswith(f"{name}: {region} written: row "), bad
        where = {"before-band": "row -1 column", "padding column": f"row {a.rows - 1} column {n} ", "after-band": f"row {a.rows} column 0 "}
        assert where[region] in bad[0] and bad[0].endswith("kernel oracle[pulse]"), bad
        with pytest.raises(AssertionError, match=f"{name}: {region} written"):
            guard.assert_only_owned_changed(before, guard.snapshot())
        a.raw[at] ^= 0xFF
        # a byte of an owned column is the library's to change
        a.raw[a.lead * a.itemsize] ^= 0xFF
        assert guard.violations(before, guard.snapshot()) == []
        a.raw[a.lead * a.itemsize] ^= 0xFF


def test_checker_names_a_write_to_a_read_only_row():
    env = make_env(65, 128, "rows", "cpu")
    scenario(env)
    guard = guarded(env)
    for name in ("_geom_f64", "_geom_i32", "_envp_rows", "_wmat_rows"):
        a = guard.arenas[name]
        before = guard.snapshot()
        a.raw[a.lead * a.itemsize] ^= 0xFF
        bad = guard.violations(before, guard.snapshot())
        assert len(bad) == 1 and bad[0].startswith(f"{name}: read-only column written: row 0 column 0 "), bad
        a.raw[a.lead * a.itemsize] ^= 0xFF


@pytest.mark.parametrize("n,stride", [(65, 65), (100, 100), (65, 66)])
def test_relaying_to_another_stride_keeps_the_owned_columns_on_the_oracle(n, stride):
    for form, segs in (("base", 129), ("rows", 128)):
        env, twin = make_env(n, segs, form, "cpu"), make_env(n, segs, form, "cpu")
        scenario(env), scenario(twin)
        want = owned_bytes(twin)
        guard = guarded(env, stride=stride)
        st = env.state
        assert st.stride == stride and st.T.shape[1:] == (stride, 4) and st.f64.shape[1] == stride and st.b.shape[1] == stride
        assert owned_bytes(env) == want
        assert torch.equal(st.workpiece_position, twin.state.workpiece_position) and st.workpiece_position.numel() == n
        run_case(env, twin, guard)                # ... and through launches and resets at that stride


# ------------------------------------------------------------------------------------------------------ GPU part
# (kernel, lanes) -> [(num_envs, segments)]: each pair's nastiest batch sizes (module docstring) on the wires it accepts
# (kernels 7, 12 and (8, 4): at most 128 segments; one or two lanes per environment put 400 segments in no LDS image)
PAIRS = {
    (1, 0): [(65, 128), (100, 400), (5, 129)], (5, 0): [(1, 128), (65, 400)], (6, 0): [(65, 128), (100, 400)],
    (6, 4): [(5, 128), (65, 129)], (6, 16): [(5, 128), (49, 400)], (2, 0): [(65, 128), (100, 400)],
    (3, 1): [(65, 128), (100, 128)], (3, 2): [(1, 128), (100, 128)], (3, 4): [(25, 128), (65, 129)],
    (3, 8): [(5, 128), (49, 400)], (3, 16): [(5, 128), (65, 400)], (4, 1): [(65, 128), (100, 128)],
    (4, 2): [(49, 128), (100, 128)], (4, 4): [(25, 128), (65, 400)], (4, 8): [(5, 128), (49, 400)],
    (10, 0): [(1, 128), (65, 400)], (2, 4): [(25, 128), (65, 129)], (2, 16): [(5, 128), (100, 400)],
    (9, 4): [(25, 128), (49, 400)], (9, 8): [(25, 400), (49, 128)], (11, 4): [(25, 128), (49, 400)],
    (11, 8): [(49, 128), (65, 400)], (11, 16): [(5, 128), (25, 400)],
    (7, 0): [(65, 128), (100, 128)], (7, 1): [(1, 128), (65, 128)], (7, 2): [(5, 128), (100, 128)],
    (8, 0): [(5, 129), (65, 400)], (8, 4): [(5, 128), (100, 128)], (8, 16): [(5, 400), (65, 129)],
    (12, 0): [(25, 128), (49, 128), (65, 128)], (0, 0): [(1, 128), (100, 400), (65, 129)],
}
assert set(KERNELS + SERVED + SERVED_ANY + [(7, 0), (7, 1), (8, 0), (8, 4), (8, 16), (12, 0), (0, 0)]) <= set(PAIRS)
CASES = [(v, l, n, s) for (v, l), shapes in PAIRS.items() for n, s in shapes]


def gpu_pair(n, segs, form, stride=None):
    gpu, cpu = make_env(n, segs, form, "cuda:0"), make_env(n, segs, form, "cpu")
    scenario(gpu), scenario(cpu)
    return gpu, cpu, guarded(gpu, stride=stride)


def assert_ran(variant, ran):
    """The shapes of this file are chosen so that every forced kernel accepts every launch: the single microsecond and both
    fused launches ran, none was refused as unsupported (and each ran the forced family: `run_case`)."""
    assert sorted(ran) == sorted(LAUNCHES), f"kernel {variant}: launches that ran: {ran}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant,lanes,n,segs", CASES)
def test_every_kernel_writes_only_the_owned_columns(variant, lanes, n, segs):
    gpu, cpu, guard = gpu_pair(n, segs, "base")
    gpu.set_kernel(variant, lanes)
    ran, _ = run_case(gpu, cpu, guard, variant, lanes, expect=FAMILY.get(variant))
    assert_ran(variant, ran)
    print(f"kernel ({variant}, {lanes}) n={n} S={segs}: " + "; ".join(f"{k} us: {v}" for k, v in ran.items())
          + "".join(f"; {k} us: unsupported" for k in LAUNCHES if k not in ran))


FORMS = [("pulse", k) for k in [(7, 0), (8, 0), (2, 4), (1, 0)]] + [("rows", k) for k in [(2, 8), (1, 0)]] + \
        [("f64", k) for k in [(7, 0), (8, 0), (2, 4), (3, 8), (6, 0), (1, 0)]] + \
        [("trace", k) for k in [(1, 0), (2, 4), (3, 8), (4, 4), (6, 0), (7, 0), (8, 0), (9, 8)]] + \
        [("keep", k) for k in [(1, 0), (2, 4), (3, 8), (4, 4), (7, 0), (8, 0)]]


@pytest.mark.gpu
@pytest.mark.parametrize("form,kernel", FORMS)
def test_every_optional_writer_writes_only_what_it_owns(form, kernel):
    """The in-launch reset, the reward and a crater ring that wraps (every case here and above), the pulse block, the
    per-environment rows (read-only), the float64 typing, a trace window strictly inside the batch whose ring wraps, and
    stepping on after termination."""
    n, segs = 65, 128
    variant, lanes = kernel
    gpu, cpu, guard = gpu_pair(n, segs, form)
    gpu.set_kernel(variant, lanes)
    launches, expect = LAUNCHES, FAMILY[variant]
    if form == "trace":
        tg, tc = (e.bind_trace(["voltage", "time", "spark_state"], every=3, capacity=5, envs=(7, 9), wire_temperature=True)
                  for e in (gpu, cpu))
        guard.guard_trace(tg)
        if variant == 9:   # (no trace point in the served kernel: a launch with a sample takes its walk unserved)
            expect = lambda k: FAMILY[9] if k == 1 else FAMILY[4]
    if form == "f64" and variant == 6:
        launches = (1, 1, 1)                                          # (the stream kernel's float64 typing: single microseconds)
    ran, _ = run_case(gpu, cpu, guard, variant, lanes, launches=launches, expect=expect)
    assert len(ran) == len(set(launches)), ran
    if form == "f64":
        assert all("[f64 stencil]" in name for name in ran.values()), ran
    if form == "trace":
        assert tg.count == tc.count == 1108 // 3 and tg.count > tg.capacity
        a, b = tg.read(), tc.read()
        assert all(torch.equal(a[k].cpu(), b[k]) for k in b)


@pytest.mark.gpu
def test_crater_ring_wrapped_and_terminations_ran_in_the_shared_scenario():
    """What the cases above rely on: in the scenario's three launches the crater ring of 8 wraps, environments terminate
    inside a launch, and the second launch resets the ones the first microsecond terminated."""
    gpu, cpu, guard = gpu_pair(65, 128, "base")
    acts = gpu.make_action(*ACTION)
    for k in LAUNCHES:
        gpu.step_many(acts, k)
    assert int(gpu.state.spark_count.max()) > 8 and int(gpu.state.episode.max()) == 1 and int(gpu.state.done.sum()) >= 13


def replay_table(n_steps, height):
    rng = np.random.default_rng(3)
    t = rng.uniform(0.0, 1.0, (n_steps, 5))
    t[:, 3] = rng.uniform(0.0, height, n_steps)
    t[:, 4] = rng.uniform(500.0, 5000.0, n_steps)
    return t


@pytest.mark.gpu
def test_injected_variates_leave_the_replay_table_alone():
    """Kernel 1's REPLAY form (the oracle's seam has none: the memory check only)."""
    n = 65
    gpu = make_env(n, 128, "base", "cuda:0")
    scenario(gpu)
    guard = guarded(gpu)
    gpu.bind_rng_replay(replay_table(1200, gpu.config.workpiece_height))
    table = gpu._replay.clone()
    ran, _ = run_case(gpu, None, guard, 1, 0, expect=FAMILY[1])
    assert sorted(ran) == [1, 7, 1100]
    assert torch.equal(gpu._replay.view(torch.int64), table.view(torch.int64)), "the replay table was written"


# ---------------------------------------------------------------------------------------------------- stride part
STRIDE_KERNELS = [(1, 0), (7, 0), (8, 0), (9, 8), (4, 4), (3, 8), (6, 0), (5, 0), (2, 8)]
_default_stride_runs = {}


def default_stride_run(variant, lanes, n, form):
    """The owned columns after every step of the same kernel at the default stride (once per kernel and batch)."""
    key = (variant, lanes, n, form)
    if key not in _default_stride_runs:
        gpu, cpu, guard = gpu_pair(n, 128, form)
        gpu.set_kernel(variant, lanes)
        _default_stride_runs[key] = run_case(gpu, cpu, guard, variant, lanes, expect=FAMILY[variant])
    return _default_stride_runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("n,stride", [(65, 65), (65, 66), (100, 100)])
@pytest.mark.parametrize("variant,lanes", STRIDE_KERNELS)
def test_strides_that_are_no_multiple_of_64(variant, lanes, n, stride):
    """Item 3 of the contract: the same launches at ``stride = num_envs`` and ``num_envs + 1`` (kernel 2 on re-laid
    per-environment geometry rows): nothing outside the owned columns is written, the owned columns equal the oracle's and,
    byte for byte, the default stride's."""
    form = "geom" if variant == 2 else "base"
    gpu, cpu, guard = gpu_pair(n, 128, form, stride=stride)
    assert gpu.state.stride == stride and gpu.state.T.shape[1] == stride
    gpu.set_kernel(variant, lanes)
    ran, stages = run_case(gpu, cpu, guard, variant, lanes, expect=FAMILY[variant])
    assert_ran(variant, ran)
    ran64, stages64 = default_stride_run(variant, lanes, n, form)
    assert ran == ran64 and stages == stages64
